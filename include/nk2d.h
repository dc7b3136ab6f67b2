/*
 * nk2d.h -- C ABI of libnk2d.so, the MI355X (gfx950) implementation of the
 * py_driver_2d Krylov / finite-difference-JVP hot path of
 * klindsay28/Newton-Krylov_OOC.
 *
 * Every entry point replaces one piece of the reference's Python plugin surface
 * (paths relative to the reference tree):
 *
 *   nk2d_create / nk2d_destroy      class-level set-up of the processes,
 *                                   nk_ooc/py_driver_2d/model_state.py:44-65
 *   nk2d_set_region                 region_mask / grid_weight / region mean matrix,
 *                                   nk_ooc/model_config.py:249-315
 *   nk2d_vec_*                      one tracer module's values (tracer, depth, ypos),
 *                                   nk_ooc/tracer_module_state_base.py:400-440
 *   nk2d_tend                       TracerModuleState.comp_tend + iage / forced / phosphorus.comp_tend,
 *                                   nk_ooc/py_driver_2d/tracer_module_state.py:98-108,
 *                                   py_driver_2d/iage.py:22-41, forced.py:114-154, phosphorus.py:58-89
 *   nk2d_vmix_coeff                 VertMix.mixing_coeff, py_driver_2d/vert_mix.py:44-101
 *   nk2d_jacobian_diags             comp_jacobian (five diagonals of the CSR matrix),
 *                                   py_driver_2d/tracer_module_state.py:262-270, iage.py:43-64
 *   nk2d_comp_fcn                   ModelState.comp_fcn's solve_ivp("Radau") year,
 *                                   nk_ooc/py_driver_2d/model_state.py:95-121
 *   nk2d_comp_fcn_hist              the same year with the 61-sample dense output of the history
 *                                   file, py_driver_2d/model_state.py:80-83,141-233
 *   nk2d_set_lin_state / nk2d_jacobian_apply
 *                                   comp_jacobian(time, tracer_vals) @ v for state dependent modules,
 *                                   py_driver_2d/phosphorus.py:105-172
 *   nk2d_precond_setup/apply        iage.apply_precond_jacobian, py_driver_2d/iage.py:66-93 (also
 *                                   forced.apply_precond_jacobian, forced.py:204-241)
 *   nk2d_precond_setup_states       the same with the tracer of the three time levels it reads from the
 *                                   precond file, forced.py:222-236 (file source with a sink threshold)
 *   nk2d_shift_factor/solve         sp_linalg.spsolve(mat - shift * mat_id, .) and the solves inside
 *                                   sp_linalg.eigs of phosphorus.apply_precond_jacobian,
 *                                   py_driver_2d/phosphorus.py:233-255
 *   nk2d_precond_setup_states on a phosphorus context (the null vector): the rest of
 *                                   phosphorus.apply_precond_jacobian per vector (extrapolation to zero shift, projection
 *                                   along the null vector), phosphorus.py:257-274: with it nk2d_precond_apply is the
 *                                   phosphorus preconditioner in one call
 *   nk2d_dot                        TracerModuleStateBase.dot_prod (weighted region mean),
 *                                   nk_ooc/tracer_module_state_base.py:379-388
 *   nk2d_axpby / nk2d_scale / nk2d_diff_scale
 *                                   state algebra with region-broadcast scalars,
 *                                   nk_ooc/tracer_module_state_base.py:200-369,502-515
 *   nk2d_lin_comb                   model_state_base.lin_comb, nk_ooc/model_state_base.py:619-624
 *   nk2d_mgs                        ModelStateBase.mod_gram_schmidt, model_state_base.py:365-377
 *   nk2d_apply_region_mask          TracerModuleStateBase.apply_region_mask, :494-500
 *
 * Conventions: plain C, no exceptions cross the boundary.  Functions return 0 on
 * success and a negative code on failure; nk2d_last_error(ctx) gives the message.
 * The caller owns every host buffer.  Host arrays are contiguous fp64, C order
 * (tracer, depth, ypos) for states and (depth, ypos) for planes.  A context owns
 * one HIP stream on one device; calls on one context are not thread safe,
 * different contexts may be driven concurrently (one per GPU / tracer module).
 * All arithmetic is IEEE fp64.
 */
#ifndef NK2D_H
#define NK2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nk2d_ctx nk2d_ctx;
/* device-resident state vector of one tracer module (opaque device pointer) */
typedef void* nk2d_vec;

#define NK2D_MAX_TRACERS 4
#define NK2D_MAX_SHIFTS 4
/* doubles per accepted step of a schedule: t, t_new, h, n_newton, t_jac, h_lu, err, fingerprint.
   err: the error-estimate norm the step was accepted with (0 in a schedule from elsewhere);
   fingerprint: nk2d_schedule_fingerprint of the context that recorded the step (0: a schedule from elsewhere, e.g.
   SciPy's steps for the step-replay parity tests -- never checked) */
#define NK2D_SCHED_WIDTH 8

typedef struct nk2d_desc {
    int32_t nz;            /* depth levels */
    int32_t ny;            /* ypos levels */
    int32_t tc;            /* tracers in the module (iage: 2) */
    int32_t device_id;     /* HIP device ordinal */
    const double* depth_edges; /* [nz+1] */
    const double* ypos_edges;  /* [ny+1] */
    const double* vvel;        /* [nz][ny+1]  Advection.vvel */
    const double* wvel;        /* [nz+1][ny]  Advection.wvel */
    const double* hmix_coeff;  /* [nz][ny-1]  HorizMix._mixing_coeff (includes 1/dy) */
    const double* bldepth_max; /* [ny]  VertMix.bldepth's bldepth_max profile */
    double bldepth_min;        /* 35 m */
    double bld_tvals[4];       /* knots of the seasonal fraction, seconds */
    double bld_fvals[4];       /* values at the knots (0,1,1,0) */
    double vmix_log_shallow;   /* ln(10)    */
    double vmix_log_deep;      /* ln(5e-4)  */
    double vmix_half_width;    /* 20 m      */
    /* module sources (iage.py:31-39, forced.py:114-139):
       tend[tr][0][:] += surf_rate[tr]*(surf_target[tr] - c[tr][0][:]);
       tend -= decay_rate[tr]*c everywhere; tend += const_src */
    double surf_rate[NK2D_MAX_TRACERS];
    double surf_target[NK2D_MAX_TRACERS];
    double decay_rate[NK2D_MAX_TRACERS];
    double const_src;
    double t0, t1;             /* time_range, seconds */
    double rtol, atol;         /* Radau tolerances (1e-6, 1e-6) */
    double max_step_frac;      /* max_step = frac*(t1-t0) (0.01) */
    double lin_tol;            /* target relative accuracy of the inner line-relaxation solves */
    /* module kind: 0 = linear sources above (iage, forced); 2 = forced with forcing files (below);
       1 = phosphorus (po4, dop, pop;
       nk_ooc/py_driver_2d/phosphorus.py:17-172), then tc = 3 and
       phos_params = {po4_halfsat, max_uptake_rate, sigma, dop_remin_rate, pop_remin_rate,
       pop_sink_vel} (phosphorus.py:42-58), light_lim [nz][ny] (phosphorus.py:26-29) */
    int32_t module_kind;
    int32_t reserved0;
    double phos_params[6];
    const double* light_lim;
    /* module kind 2 = forced module with file-driven forcing (nk_ooc/py_driver_2d/forced.py:42-56,
       125-153,188-202): tc = 1.  The records are the file's fields already interpolated to the
       model axes (nk_ooc/utils.py:488-533); the library interpolates them linearly in time with
       linear extrapolation beyond the first / last record, as scipy's interp1d(fill_value=
       "extrapolate") does.  restore_nrec > 0: tend[0][0][:] += surf_rate[0]*(restore(t) - c[0][:])
       with restore(t) from the records instead of surf_target[0].  sms_nrec > 0: tend += sms(t),
       and with sink_thres > 0 sms is multiplied by c/sink_thres where sms < 0 and 0 < c/sink_thres < 1
       (then the Jacobian has the state-dependent diagonal of forced.py:188-202).  decay_rate[0] and
       const_src keep their meaning (forced_sms_opt = decay / const). */
    int32_t restore_nrec;
    int32_t sms_nrec;
    const double* restore_times; /* [restore_nrec], seconds, increasing */
    const double* restore_vals;  /* [restore_nrec][ny] */
    const double* sms_times;     /* [sms_nrec] */
    const double* sms_vals;      /* [sms_nrec][nz][ny] */
    double sink_thres;           /* 0: no threshold */
} nk2d_desc;

typedef struct nk2d_stats {
    int64_t nfev, njev, nlu;       /* SciPy-compatible counters */
    int64_t nsteps, nrejected;     /* accepted steps, rejected attempts */
    int64_t nnewton, nsolve;       /* Newton iterations, linear solves */
    int64_t nsweeps;               /* line-relaxation sweeps (kernel launches) */
    int64_t nlaunch;               /* total kernel launches */
    double seconds;                /* host wall time of the call */
    int64_t nresumed;              /* frozen year: times it was resumed from a checkpoint with one more Newton iteration */
    int64_t nerr_checked;          /* frozen year: steps whose error estimate was evaluated (option "frozen_err_check") */
    double max_err;                /* ... and the largest of them (SciPy accepts a step at <= 1) */
    int64_t nbarrier_timeouts;     /* 1: the one-launch year timed out at a grid barrier and was rerun under host control */
} nk2d_stats;

int nk2d_create(const nk2d_desc* desc, nk2d_ctx** out);
void nk2d_destroy(nk2d_ctx* ctx);
const char* nk2d_last_error(const nk2d_ctx* ctx);
const char* nk2d_version(void);

/* region_mask [nz][ny] (int32, 0 = outside), grid_weight [nz][ny]; nreg = max(mask) */
int nk2d_set_region(nk2d_ctx* ctx, const int32_t* mask, const double* weight, int32_t nreg);

int nk2d_vec_alloc(nk2d_ctx* ctx, nk2d_vec* out);
int nk2d_vec_free(nk2d_ctx* ctx, nk2d_vec v);
int nk2d_vec_upload(nk2d_ctx* ctx, nk2d_vec v, const double* host);   /* [tc][nz][ny] */
int nk2d_vec_download(nk2d_ctx* ctx, nk2d_vec v, double* host);
/* The same in two halves, for a caller that writes vector files on a thread of its own (what the reference does inside
 * ModelStateBase.dump, nk_ooc/model_state_base.py:93-111, here behind the next forward year): `begin` queues the copy
 * into a pinned buffer of the download's own on the context's stream and returns at once (later work on the stream,
 * including changes of v, is ordered behind it); `end` -- on any host thread -- waits for that copy alone and fills
 * host [tc][nz][ny] (NULL: only releases the ticket).  Every ticket must be ended once, before nk2d_destroy. */
int nk2d_vec_download_begin(nk2d_ctx* ctx, nk2d_vec v, void** ticket);
int nk2d_vec_download_end(nk2d_ctx* ctx, void* ticket, double* host);
int nk2d_vec_copy(nk2d_ctx* ctx, nk2d_vec dst, nk2d_vec src);
int nk2d_vec_zero(nk2d_ctx* ctx, nk2d_vec v);

/* deterministic kernels */
int nk2d_tend(nk2d_ctx* ctx, double t, nk2d_vec y, nk2d_vec f);
int nk2d_vmix_coeff(nk2d_ctx* ctx, double t, double* host_out /* [nz-1][ny] */);
/* state the stand-alone Jacobian entry points below linearise about (only state dependent
   modules, i.e. phosphorus, use it); nk2d_comp_fcn linearises about its own running state */
int nk2d_set_lin_state(nk2d_ctx* ctx, nk2d_vec y);
/* out = J(t, lin_state) v : tracer_module.comp_jacobian(...) @ v,
   py_driver_2d/tracer_module_state.py:262-270, phosphorus.py:105-172 */
int nk2d_jacobian_apply(nk2d_ctx* ctx, double t, nk2d_vec v, nk2d_vec out);
/* diags: [5][tc][nz][ny] in the order up(k-1), south(j-1), centre, north(j+1), down(k+1) */
int nk2d_jacobian_diags(nk2d_ctx* ctx, double t, double* host_out);
/* solve ((mu/h) I - J(t_jac)) x = b by line relaxation; complex when mu_im != 0.
   b_re/b_im/x_re/x_im are device vectors (b_im, x_im ignored for real systems). */
int nk2d_shifted_solve(nk2d_ctx* ctx, double t_jac, double h, double mu_re, double mu_im,
                       nk2d_vec b_re, nk2d_vec b_im, nk2d_vec x_re, nk2d_vec x_im,
                       int32_t* sweeps_out);

/* one forward year: fx = y(t1) - x, region-masked.
   replay: optional schedule [replay_n][NK2D_SCHED_WIDTH] to consume (step-replay mode; the inner
           tolerance is then min(lin_tol, 1e-3): the schedule fixes the Newton iteration counts);
   record: optional buffer [record_cap][NK2D_SCHED_WIDTH] receiving the accepted steps. */
int nk2d_comp_fcn(nk2d_ctx* ctx, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats,
                  const double* replay, int64_t replay_n,
                  double* record, int64_t record_cap, int64_t* record_n);
/* The finite-difference product of the reference, (F(x + sigma v) - F(x)) / sigma with sigma = 1e-4 |x|
   (model_state_base.py:492-527), differences two years of an ADAPTIVE integrator: wherever the two controllers
   decide differently (a rejected step, another Newton iteration) the difference of their discretisation errors,
   divided by sigma, lands in the product -- measured here at 5 % ... 90 % of |w| for the first Krylov direction, in
   every controller mode including SciPy's own (tools/probe_jvp_noise.py).  Internal numerical differentiation removes
   it: the perturbed year repeats the accepted steps, Newton iteration counts, Jacobian times and factorisations of
   the year that produced F(x), which makes w the derivative of ONE discrete map.
   nk2d_comp_fcn_frozen: forward year on a schedule recorded by nk2d_comp_fcn on this context under the same options,
   with the recorded year's own inner tolerance, nothing decided and nothing read back (for the recorded x itself it
   reproduces the recorded year bit for bit).
   nk2d_set_frozen_schedule: the schedule the perturbed years of nk2d_jvp / nk2d_gmres_solve repeat from now on
   (copied; sched_n = 0 returns them to free-running years). */
int nk2d_comp_fcn_frozen(nk2d_ctx* ctx, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, const double* sched, int64_t sched_n);
int nk2d_set_frozen_schedule(nk2d_ctx* ctx, const double* sched, int64_t sched_n);
/* A frozen year checks afterwards, for every step, SciPy's Newton convergence test on the last recorded iteration
   (with a slack of 30) -- the norm partials of those iterations are kept, one reduction launch and one read-back per year.
   Where the recorded count is not enough for the state given, the year is RESUMED from the checkpoint before the first
   such step (the state is kept every 128 steps) with one more Newton iteration there, at most twice; a year that still
   fails -- or a step already at SciPy's six iterations -- makes nk2d_comp_fcn_frozen return -7, and nk2d_jvp then runs a
   free-running year instead.  Option "frozen_err_check" k > 0 (default 128: the steps that open a checkpoint interval) also evaluates SciPy's
   error estimate on every k-th step of a frozen year (one launch each, plus the tendency at the step start): a step whose estimate
   exceeds 1.5 * max(1, recorded estimate) returns -7 as well.  A schedule whose fingerprint is not this context's
   (other options, grid or library build) is refused with -8 before anything runs.
   nk2d_frozen_fallbacks: how often a frozen year was given up (-7) on this context (and how often a one-launch year of option
   "frozen_phosphorus" was handed back to the launch-per-phase path because a hand-over timed out); nk2d_frozen_resumes: how often one was
   resumed. */
int nk2d_frozen_fallbacks(nk2d_ctx* ctx, int64_t* n);
int nk2d_frozen_resumes(nk2d_ctx* ctx, int64_t* n);
/* Modules whose Jacobian is a function of time alone, grids of up to 512 levels (option "frozen_persistent_max_e", levels per
   lane, default 8; five to eight only with linear sources): a frozen year runs as ONE launch whose workgroups are all resident -- a wave or a
   four-wave team per column, one simplified-Newton iteration per phase, workgroups handing over to their lateral neighbours
   between phases -- on a cache of everything its schedule fixes besides the state: mixing planes, Jacobian planes and line
   factorisation of every step, built by two batched launches when a new schedule arrives (options "frozen_persistent" 0/1,
   "frozen_cache_gb": at most that much HBM, default 128, and never more than 85 % of what the device has free; 102 GB and 26 ms
   per schedule at 416 x 416, where the year takes 115 - 120 ms instead of 190 ms; "frozen_cache_after": frozen years of a schedule
   that run launch by launch before its cache is built, default 0; "frozen_alloc_async" 1, default: a cache above 8 GB is
   allocated by a thread of the library's own -- hipMalloc of 120 GB takes 0.03 to 3 s -- and the years of the meantime run
   launch by launch; "frozen_cache_pieces" 0, default, or 1, opt-in: the cache is a list of equally sized pieces, one hipMalloc
   each, instead of one slab -- piece p holds rows [p B, (p + 1) B) laid out as a slab of B rows, B = max(1, floor(
   "frozen_cache_piece_mb" MiB / bytes of a row)), default 1024 MiB, or "frozen_cache_piece_rows" (default 0: unset) directly; a
   schedule of n rows needs ceil(n / B) pieces, pieces are kept from schedule to schedule and only added to, the limits above
   apply to their sum, the thread allocates piece by piece and all its pieces are adopted together, switching the option frees
   the other form first; "frozen_cache_early" 0, default, or 1, with pieces only: nk2d_comp_fcn with `record` asks the thread for
   the pieces of the schedule it recorded when the year ends, whatever their size; "frozen_cache_lean" 0, default, 1 or 2, opt-in,
   read when a cache is (re)built: the cache holds the mixing and Jacobian planes only -- 8 n (3 kv_len + 5 np) bytes, about 30 % of
   the full rows, to which every limit above then applies -- and the year factorises in the first phase of every step, on one
   row's worth of factor tables; 1: every schedule cache of the context, 2: only a schedule whose full cache "frozen_cache_gb" or
   the 85 % rule would refuse; composes with pieces, switching lean <-> full frees the other form first, any other value is an
   error, not taken with "factor_fp32"; "frozen_forced" (environment NK2D_FROZEN_FORCED), a bit mask, default 0, opt-in, read at
   every frozen year: the one-launch year for the file-driven forced module (module_kind 2) where it has none by default -- bit 1:
   without a sink threshold at five to eight levels per lane, on the full or the lean cache, slab or pieces; bit 2: WITH a sink
   threshold (sink_thres > 0, whose Jacobian reads the state through one diagonal plane) at one to eight levels per lane, on the
   lean cache only ("frozen_cache_lean" 1, or 2, which for such a context always means lean; with 0 the year routes as without
   the option): a row of that cache also holds the file-source plane at its Jacobian time, 8 n (3 kv_len + 5 np + np) bytes, and
   the year forms that diagonal plane for each wave's own column, from the state at the step start, at the rows where the
   launch-per-phase path evaluates the Jacobian anew, in a plane the cache owns; any value outside 0 ... 3 is an error; phosphorus
   contexts are unaffected; "frozen_phosphorus" (environment NK2D_FROZEN_PHOSPHORUS), default 0, opt-in, read at every frozen
   year: the one-launch year for the phosphorus module (module_kind 1, whose Jacobian reads the state through one diagonal plane and
   whose tracers are coupled inside a ypos column), at three to eight levels per lane, on the lean cache only ("frozen_cache_lean" 1,
   or 2, which for such a context always means lean; with 0 the year routes as without the option), a row of which is the planes
   alone, 8 (3 kv_len + 5 np) bytes: the workgroup is one ypos column with its tracers, a wave each, whatever "frozen_by_column" and
   "frozen_coef_lds" say, and every wave forms that diagonal plane for the column, from the state at the step start, at the rows
   where the launch-per-phase path evaluates the Jacobian anew, in a plane the cache owns -- 1: the kernel at one wave per SIMD
   where all its workgroups are resident, otherwise the year routes on as without the option; 2: as 1, and where that flavour is
   not resident the same kernel within 256 registers (two waves to a SIMD, five to eight levels per lane) if that one is; 3: the
   256-register flavour wherever it exists; any value outside 0 ... 3 is an error; one and two levels per lane stay out: the
   by-column workgroup does not exist there and a four-wave team cannot hold three coupled tracers; other modules are unaffected;
   "frozen_phosphorus_shallow" (environment NK2D_FROZEN_PHOSPHORUS_SHALLOW), 0, default, or 1, opt-in, read at every frozen year:
   with 1 a module_kind 1 context at ONE and TWO levels per lane (up to 128 depth levels: the grids the model is shipped with) takes
   the one-launch year too, where "frozen_phosphorus" is non-zero and "frozen_cache_lean" is 1 or 2 -- the same workgroup of one
   ypos column with its tracers, a wave each and never a team, nothing of the year in LDS, the one-wave flavour whatever the value of
   "frozen_phosphorus"; everything else as at three to eight levels per lane; with 0 every year of every context takes the path it
   takes without the option; the option changes no bit of a year, so the schedule fingerprint does not take it in; any other value
   is an error).
   Same device functions, bit-identical results; a year that does not pass the Newton check, or a
   barrier that times out, is handed to the launch-per-phase path.  Counters by name: "frozen_persistent_years",
   "frozen_team_years" (of them: a four-wave team per column), "frozen_cache_bytes",
   "frozen_launch_us" (device time of those launches), "frozen_cache_pending" (1 while a thread allocates a large cache or pieces),
   "frozen_cache_pieces" (pieces held; "frozen_cache_bytes" is then their sum), "frozen_cache_piece_allocs" (pieces allocated
   so far), "frozen_cache_early_requests" (early requests made), "frozen_cache_lean" (1 while the cache held is lean),
   "frozen_lean_years" (one-launch years run on a lean cache; also counted in "frozen_persistent_years"),
   "frozen_lds_bits" (the bits of option "frozen_coef_lds" in effect in the one-launch year launched last, after fitting),
   "frozen_early_bits" (option "frozen_early" as in effect in that year: 0 wherever "frozen_lds_bits" lacks 16 and 32),
   "frozen_stage_exchange_bits" (option "frozen_stage_exchange" as in effect in that year, under the same rule -- and 0 whatever the
   option says for linear sources at seven levels per lane on a cache in pieces, whose kernel has no body for it),
   "frozen_xlane_bits" (option "frozen_xlane" as in effect in that year: 0 wherever "frozen_stage_exchange_bits" is 0),
   "frozen_dedicated_bits" (option "frozen_dedicated" as in effect in that year: 1 or 2 only where the year ran in the kernel that
   carries the default year's body alone), "frozen_dedicated_years" (one-launch years that kernel ran; also counted in
   "frozen_persistent_years"),
   "frozen_step_sums_hash" (64-bit FNV-1a hash of the bits of the step sums the last whole-year check of a frozen year read: the
   norm sums of every step's last Newton iteration and of the one before -- the same for the same year by whatever path),
   "frozen_forced_years" (one-launch years only option "frozen_forced" made possible; also counted in "frozen_persistent_years",
   and in "frozen_lean_years" where lean),
   "frozen_phosphorus_years" (one-launch years of the phosphorus module, option "frozen_phosphorus"; also counted in
   "frozen_persistent_years" and "frozen_lean_years"), "frozen_two_waves_years" (of them: the years that ran the 256-register flavour),
   "frozen_phosphorus_shallow_years" (one-launch years only option "frozen_phosphorus_shallow" made possible: phosphorus at one and
   two levels per lane; also counted in "frozen_phosphorus_years", "frozen_persistent_years" and "frozen_lean_years", never in
   "frozen_team_years" or "frozen_two_waves_years"),
   "frozen_cache_builds", "frozen_fallbacks", "frozen_resumes"; of the host-side controller: "spec_launches_dropped",
   "spec_front_launches_dropped", "err_estimates_queued", "err_estimates_dropped" (work queued ahead of a verdict); of the
   preconditioner (option "pc_two_ended"): "pc_setup_rounds" (dependent inversion rounds of the last block elimination: ny,
   or ny / 2 + 1 from both ends), "pc_sub_launches" (dependent mat-vec launches of the last block substitution: 2 ny - 1,
   or at most ny + 2); (option "pc_pivot_wave") "pc_pivot_wave_steps" (panel steps of the last block elimination that ran
   a one-wave pivot inversion: 0, or ceil(m / 32) * "pc_setup_rounds"); (option "pc_panel") "pc_panel_steps" (64-wide panel
   steps of the last block elimination: 0 with the option at 32, ceil(m / 64) * "pc_setup_rounds" at 64);
   "pc_phos_applies" (nk2d_precond_apply calls of this context that ran the one-call phosphorus preconditioner,
   the null-vector form of nk2d_precond_setup_states). */
int nk2d_get_counter(nk2d_ctx* ctx, const char* name, int64_t* out);
/* hash of everything a recorded schedule depends on besides the state: grid, module description, tolerances, the
   controller options (jac_fresh, jac_stage, lin_tol, min_sweeps, growth_cap, factor storage), the library version and a
   checksum of its sources (another build's schedules are refused);
   an integer below 2^52, never 0 */
int nk2d_schedule_fingerprint(nk2d_ctx* ctx, double* out);
/* accepted steps of the most recent free-running year of this context (whichever entry point ran it: nk2d_comp_fcn,
   nk2d_comp_fcn_hist, the perturbed year of a free-running nk2d_jvp): n rows of NK2D_SCHED_WIDTH doubles; out may be
   NULL to ask for n only */
int nk2d_last_schedule(nk2d_ctx* ctx, double* out, int64_t cap, int64_t* n);

/* the same forward year with dense output: the solution at the n_eval increasing times t_eval
   (within [t0, t1]) is written to host_hist [n_eval][tc][nz][ny], evaluated from each step's
   collocation polynomial as solve_ivp(t_eval=...) does (the 61-sample history of
   py_driver_2d/model_state.py:80-83) */
int nk2d_comp_fcn_hist(nk2d_ctx* ctx, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, int32_t n_eval,
                       const double* t_eval, double* host_hist);

/* preconditioner  M^-1 v = (I - prod_k (I - dt J(t_k)))^-1 v - v */
int nk2d_precond_setup(nk2d_ctx* ctx);
/* the same for a forced module whose Jacobian depends on the state (file source with sink_thres):
   states[i] = the tracer at the end of the i-th third of [t0, t1], as forced.apply_precond_jacobian
   reads it from the preconditioner file (py_driver_2d/forced.py:222-236).
   On a phosphorus context (module_kind 1) the call takes ONE vector, states[0] = e_hat, and completes the set-up of the
   extrapolated phosphorus preconditioner of phosphorus.py:197-274 (the null-vector form; no entry point of its own, the ABI
   keeps its 56): it declares that systems 0 and 1 of the current nk2d_shift_factor factorisation are that preconditioner --
   shifts[0] = shift, shifts[1] = shift / 2 with shift = half the second smallest eigenvalue of mat = scale J -- and e_hat
   the null vector of mat scaled to unit region mean (e / <e, 1>); the context keeps a copy.  From then on
   nk2d_precond_apply and nk2d_gmres_solve work on this context.  Refused when there is no shifted factorisation or it has
   fewer than two systems, and when states or states[0] is null; on a context that is neither a forced module with forcing
   files nor phosphorus the call is refused as before.  Any later nk2d_shift_factor on the context removes the declaration,
   as would any other set-up (the storage is shared; e_hat belongs to one factorisation).  The eigen-pair itself stays above
   this boundary, where the reference has it (sp_linalg.eigs): a binding factorises mat - mu I with nk2d_shift_factor and
   hands nk2d_shift_solve to eigs as OPinv (shift-invert), as PhosphorusPrecond does with its own Arnoldi loop. */
int nk2d_precond_setup_states(nk2d_ctx* ctx, const nk2d_vec* states);
/* nk2d_precond_apply: out = M^-1 v with the preconditioner of the last set-up.  On a phosphorus context (module_kind 1) that
   is the extrapolated preconditioner declared by the null-vector form of nk2d_precond_setup_states above, the whole of
   phosphorus.apply_precond_jacobian's per-vector work (phosphorus.py:257-274) in one call: v goes into the right-hand sides
   of both shifted systems in one launch, both run down ONE block substitution chain (2 ny - 1 dependent mat-vec launches,
   at most ny + 2 with "pc_two_ended", instead of that many per system; "pc_fp32" / "pc_refine" as in nk2d_shift_solve),
   then  s = 2 A_1^-1 v - A_0^-1 v,  out = s - <s, 1> e_hat - v  region by region; nothing is read back and the host does
   not wait.  out may be v.  The result is, bit for bit, that of the five calls nk2d_shift_solve(0), nk2d_shift_solve(1),
   nk2d_axpby(2, half, -1, full), nk2d_axpby(1, s, -nk2d_dot(s, ones), e_hat), nk2d_axpby(1, ., -1, v).  Without the
   declaration a phosphorus context is refused.  Counter "pc_phos_applies": the calls of this context that took this
   path; "pc_sub_launches" is then the one chain of the call.  (PhosphorusPrecond of the Python layer uses the call with
   NK2D_PHOS_PC_FUSED=1 in the environment, read when the engine is created; default 0: the five calls.) */
int nk2d_precond_apply(nk2d_ctx* ctx, nk2d_vec v, nk2d_vec out);
/* shifted systems of the phosphorus preconditioner (phosphorus.py:233-255): factorise
   A_i = scale * J(t, lin_state) - shifts[i] * I (all tracers of the module coupled, nshift <=
   NK2D_MAX_SHIFTS) by block elimination over the ypos columns, replacing the reference's
   sp_linalg.spsolve(mat - shift * mat_id, .) and the solves inside sp_linalg.eigs(sigma=...);
   nk2d_shift_solve: out = A_i^-1 v.  Shares its storage with nk2d_precond_setup. */
int nk2d_shift_factor(nk2d_ctx* ctx, double t, double scale, int32_t nshift, const double* shifts);
int nk2d_shift_solve(nk2d_ctx* ctx, int32_t i, nk2d_vec v, nk2d_vec out);

/* state algebra; region scalars are host arrays [nreg], broadcast with fill 1.0 where mask<=0 */
int nk2d_dot(nk2d_ctx* ctx, nk2d_vec a, nk2d_vec b, double* out /* [nreg] */);
int nk2d_axpby(nk2d_ctx* ctx, nk2d_vec out, const double* a, nk2d_vec x, const double* b, nk2d_vec y);
int nk2d_scale(nk2d_ctx* ctx, nk2d_vec out, nk2d_vec x, const double* s);
int nk2d_diff_scale(nk2d_ctx* ctx, nk2d_vec out, nk2d_vec x, nk2d_vec y, const double* s);
int nk2d_lin_comb(nk2d_ctx* ctx, nk2d_vec out, int32_t n, const nk2d_vec* vecs,
                  const double* coef /* [n][nreg] */);
/* in-place modified Gram-Schmidt of w against n basis vectors; h_out [n][nreg] */
int nk2d_mgs(nk2d_ctx* ctx, nk2d_vec w, int32_t n, const nk2d_vec* basis, double* h_out);
int nk2d_apply_region_mask(nk2d_ctx* ctx, nk2d_vec v);

/* Measurement plumbing (bench.py): time every every_n-th WINDOW of the dominant kernel
   (k_newton_fused) with a HIP event pair on the context's stream.  A window is the launches of one
   simplified-Newton iteration that are queued back to back with nothing between them (first
   iteration of a step attempt).  every_n = 0 switches sampling off. */
int nk2d_profile_reset(nk2d_ctx* ctx, int32_t every_n);
/* avg_us: (window times - one empty-pair reading per window) / launches inside the windows;
   samples: those launches; windows: timed windows; bytes: algorithmic bytes of the launches in
   the windows; launches: all launches of the kernel since the reset; overhead_us: what an EMPTY
   event pair reads on this stream */
int nk2d_profile_read(nk2d_ctx* ctx, double* avg_us, int64_t* samples, int64_t* launches, double* bytes,
                      double* overhead_us, int64_t* windows);

/* the same counters since the last nk2d_profile_reset over ALL launches of the dominant kernel (timed
   or not): their number and their algorithmic bytes -- for the end-to-end rate bytes / wall time */
int nk2d_profile_totals(nk2d_ctx* ctx, int64_t* launches, double* bytes);
/* the launches of the dominant kernel without the factorisation since the last nk2d_profile_reset, by shape
   (0: stage + sweep + update, 1: stage + first sweep, 2: last sweep + update, 3: a middle sweep), and their
   algorithmic bytes */
int nk2d_profile_shapes(nk2d_ctx* ctx, int64_t* counts4, double* bytes4);
/* n launches of shape 0, 1 or 2 of that kernel queued back to back inside ONE event pair, on the state the last
   forward year left behind, their updates written to scratch: microseconds per launch (the hand-over between
   consecutive launches included, no event cost to subtract) and the algorithmic bytes of one such launch */
int nk2d_profile_replay(nk2d_ctx* ctx, int32_t shape, int32_t n, double* avg_us, double* bytes_per_launch);
/* a HIP event pair on the context's own stream for the caller's measurements (bench.py times the
   preconditioner apply with it): nk2d_timer_begin records the first event, nk2d_timer_end records
   the second, waits for it and returns the elapsed milliseconds between the two */
int nk2d_timer_begin(nk2d_ctx* ctx);
int nk2d_timer_end(nk2d_ctx* ctx, double* elapsed_ms);

/* ---- the Krylov loop itself on the device ------------------------------

   nk2d_jvp: ModelStateBase.comp_jacobian_fcn_state_prod for one tracer module,
   nk_ooc/model_state_base.py:492-527, in one call: sigma[r] = 1e-4 * norm(x)[r] (1 where that is 0),
   w = (F(x + sigma v) - fx) * (1 / sigma), region by region.  fx = F(x) is the caller's (the Newton
   solver has it).  perturb_fcn (optional, may be null) receives F(x + sigma v), the vector the
   reference dumps as perturb_fcn_w_raw_NN.nc; sigma_out (optional) [nreg]; stats (optional) of the
   perturbed forward year.  The perturbed year is a free-running one, as the reference's, unless a schedule is
   installed (nk2d_set_frozen_schedule): then it repeats the accepted steps of the year that produced fx, and a
   state the recorded Newton counts do not converge for gets a free-running year after all (nk2d_frozen_fallbacks). */
int nk2d_jvp(nk2d_ctx* ctx, nk2d_vec x, nk2d_vec fx, nk2d_vec v, nk2d_vec w, nk2d_vec perturb_fcn,
             double* sigma_out, nk2d_stats* stats);

/* nk2d_gmres_solve: KrylovSolver.solve + _solve0 for ONE tracer module, nk_ooc/krylov_solver.py:85-165:
   left-preconditioned GMRES (Saad alg. 9.4), zero initial guess, no restart, one Hessenberg per
   region, coefficients = argmin || beta e_1 - H c ||_2 (the reference calls np.linalg.lstsq,
   krylov_solver.py:168-181; here a Givens QR of the Hessenberg -- the same minimiser), stop when
   iteration >= min_iter and || sum_j c_j w_j + M^-1 fx || < rel_tol * beta in every region, or at
   max_iter.  Everything stays in HBM; nothing is written to disk (the Python mirror of KrylovSolver
   keeps the reference's file trail).  The preconditioner is nk2d_precond_apply: call
   nk2d_precond_setup (or _setup_states) first; on a phosphorus context nk2d_shift_factor with the two shifts and
   nk2d_precond_setup_states with the null vector -- without that declaration the phosphorus module is refused before any device work.
   Outputs (caller-owned host buffers, zero padded): beta [nreg]; h_mat [max_iter+1][max_iter][nreg]
   (the reference's h_mat[module] with the iteration axes first); resid_norm [max_iter][nreg];
   coeff [max_iter][nreg] of the last iteration; *iters = iterations done; increment = the device
   vector the reference dumps as increment_NN.nc.  Any of beta / h_mat / resid_norm / coeff may be null. */
int nk2d_gmres_solve(nk2d_ctx* ctx, nk2d_vec x, nk2d_vec fx, double rel_tol, int32_t min_iter,
                     int32_t max_iter, nk2d_vec increment, double* beta, double* h_mat,
                     double* resid_norm, double* coeff, int32_t* iters);

/* all n region-weighted dot products <w, basis[i]> in one launch and one read-back (the fused
   multi-dot of SURVEY.md section 8(e)); out [n][nreg] */
int nk2d_multi_dot(nk2d_ctx* ctx, nk2d_vec w, int32_t n, const nk2d_vec* basis, double* out);
/* w -= sum_i bcast(h[i]) basis[i] in one launch; h [n][nreg] (classical Gram-Schmidt update).  fill: the
   broadcast value where region_mask <= 0 -- 1.0 is the reference's (every modified Gram-Schmidt projection
   subtracts basis[i] itself there); a re-orthogonalisation pass uses 0.0 so as not to subtract it twice */
int nk2d_multi_axpy(nk2d_ctx* ctx, nk2d_vec w, int32_t n, const nk2d_vec* basis, const double* h, double fill);

/* Tracers of one module sharded over several contexts / GPUs (level 2): the
   tracers' Jacobian blocks are independent, but SciPy's Radau takes its decisions from norms over the
   whole module (radau.py:118,481; common.py:63-65).  With a hook installed, every sum of squares the
   controller reads is passed through `fn` (the caller makes it an all-reduce over the shards: RCCL on
   GPUs, gloo in the CPU tests) and the RMS norms divide by global_n = the module's tc * nz * ny, so
   that all shards take identical decisions.  fn == NULL removes the hook.  (A hooked context's years are launched: the
   controller waits for the caller's all-reduces, which no resident kernel should sit through -- option "stream_years".) */
typedef double (*nk2d_norm_hook_fn)(void* user, double local_sum_of_squares);
int nk2d_set_norm_hook(nk2d_ctx* ctx, nk2d_norm_hook_fn fn, void* user, double global_n);
/* The same with several sums per call (1 <= n <= 4; replaced in place by the module-wide sums): the controller then
   BATCHES what it can -- the norm of a Newton iteration with those of up to two iterations queued speculatively behind it
   (option "hook_spec_depth", default 2; 1 = one) and with the error estimate queued behind the iteration expected to be the
   last -- and a coupled year takes well under half the collectives of the scalar hook (measured: tools/probe_pairing.py,
   bench.py's shard_e2 leg); the decisions and their order are the scalar hook's, the schedules identical.  Unwanted
   iterations and estimates are dropped.  A context has one hook: installing either kind removes the other. */
typedef void (*nk2d_norm_hook_vec_fn)(void* user, double* sums, int32_t n);
int nk2d_set_norm_hook_vec(nk2d_ctx* ctx, nk2d_norm_hook_vec_fn fn, void* user, double global_n);

/* run-time options.  ONE set of defaults since round 3: a context is created in the mode the engines, the tests of the
   benchmarked path and bench.py run -- "jac_fresh" 1, "jac_stage" 1 (and desc.lin_tol = 3e-2 is what they pass);
   SciPy's decisions step for step are "jac_fresh" 0 + "jac_stage" -1 (what the counter-parity tests set).
   "lin_tol" (relative accuracy of the inner line-relaxation solves),
   "stream_years" (bit 1, default: free-running forward years run as COMMAND STREAMS -- one resident kernel executes the
   launches of the host-controlled year as commands pushed into a ring in HBM, workgroups hand over to their two lateral
   neighbours between commands, norm partials come back through pinned host memory; same controller, same device functions,
   the same year bit for bit, csrc/nk2d_stream.h.  Bit 2: frozen / replayed years too -- measured slower than the one-launch
   year on the schedule cache for the modules that has one, equal to launches otherwise; 0: every year by launches.
   Counters "stream_years_run", "stream_commands", "stream_launches" (kernel starts), "stream_timeouts" (kernels that gave
   up: the year is rerun by launches), "stream_prof_0..11" (microseconds per workgroup waiting for commands / executing /
   waiting for neighbours, commands, and per kind of command).  NK2D_STREAM_RELAY=1 in the environment: commands through
   pinned host memory and a relay wave instead of written over the large BAR),
   "stream_two_waves" (default 1; before the context's first year: phosphorus from five levels per lane takes the flavour of
   the resident kernel that fits two waves to a SIMD -- 256 registers, the rest in scratch memory -- where that lets every
   (tracer, ypos) column be resident instead of several rounds of columns per command, 416 x 416: 1 248 columns; 2: wherever
   that flavour exists; 0: never.  Counters "stream_two_waves_kernel", "stream_columns_per_workgroup"),
   "stream_xlane" (0, default, or 1; read at every start of the resident kernel, NK2D_STREAM_XLANE in the engines' environment:
   the kernel runs every command -- Newton, error estimate, sweep, set-up, step boundary, Jacobian -- with its cross-lane moves
   at distances 1 and 32 lanes and its sums over the wave as DPP and v_permlane32_swap in the VALU instead of ds_bpermute through
   LDS: the vertical stencil of the tendencies, of the Jacobian diagonals and of the sinking flux, the first and last levels of
   the parallel cyclic reductions of the line factorisation and of the solves, the norm partials; distances 2 to 16 stay on
   ds_bpermute.  A flavour of the kernel of its own, never a run-time flag inside today's; every lane receives the same 64 bits:
   the same year bit for bit, no decision, not part of the schedule fingerprint, no change of the kernel's shape.  Counter
   "stream_xlane_bits": what the kernel launched last ran with -- 0 for linear sources at one level per lane (no such flavour:
   it needs scratch memory where today's kernel needs none), 0 where the flavour would not keep every workgroup resident at
   the shape the context has, 0 for a year from the tape ("frozen_tape"), whose kernel has today's body only),
   "stream_hist" (0, default, or 1; opt-in: the samples of nk2d_comp_fcn_hist in a year that runs as a command stream are
   COMMANDS of its resident kernel -- the dense output of the accepted step, packed, into a slot of a sample buffer in HBM,
   pushed right behind the step's boundary command, which such a step keeps -- instead of ending the kernel for a piece of
   launches and a device-to-host copy per sample; the host unpacks and copies the buffered samples out when the slots are
   full and after the year's end.  A step that has no fused boundary command samples by launches as before -- the year's
   last step always; otherwise only a step whose t + h rounds off t_new or whose successor's step size is not a positive
   number -- and is not counted.  The same samples and the same year bit for bit; a year whose kernel gives up is rerun by
   launches, samples included, and books nothing in the two counters below),
   "stream_hist_mb" (>= 0, default 256: budget of that sample buffer in MiB; it holds
   clamp(floor(budget / bytes of a packed state), 1, samples of the year) slots, 0 means a single slot.  Counters
   "stream_hist_samples": samples produced by a command and delivered, "stream_hist_drains": times the buffer was emptied --
   both booked when a year has run as a stream to its end),
   "device_ctl" (only 0: rounds 1 - 3 had device-side controllers 1, 2, 3; they lost to the command stream and are gone),
   "spec_bias" (default 1: what the host queues behind a Newton iteration it has not judged yet -- the next iteration, or the
   error estimate when the predicted convergence test value is below this many tolerances; never a decision; measured flat),
   "jac_fresh" (1: re-evaluate the
   Jacobian at every step start instead of SciPy's reuse heuristic; same ODE, same error
   control, different -- shorter -- sequence of Newton iterations), "growth_cap" (> 0: largest
   growth factor of the step size after a step whose Newton iteration failed and was repeated with
   half the step; 1.0 is the rule of Hairer & Wanner's RADAU5, 0 = SciPy, which has none),
   "min_sweeps" (1, default: a solve whose contraction bound meets lin_tol after ONE sweep runs the whole simplified
   Newton iteration as a single launch, its update written to a spare stage buffer; 2: at least two sweeps wherever
   columns couple, the round-1 rule),
   "final_fuse" (1, default: a step of a frozen year, nk2d_comp_fcn_frozen, ends in the launch of its last Newton
   iteration; 0: in a step boundary launch of its own, for A/B runs),
   "jac_stage" (0, 1 or 2, with "jac_fresh" 1: the Jacobian of a step attempt is
   taken at the time of that stage of the attempt, t + c_i h, instead of the step start -- the simplified Newton
   iteration and the error filter use ONE Jacobian for the three stages and the vertical mixing changes over a step;
   the launch that computes the stage's mixing plane derives the Jacobian planes from it.  1 is the default; -1:
   the step start, as SciPy.  Modules whose Jacobian also reads the state take the mixing plane of that time and the
   state of the step start, in a launch of their own -- option "jac_stage_state" 1, the default; 0: step start for both),
   "team" (launch shape of the Newton-iteration launches: 0 one wave per column; 1 one workgroup of four waves per
   column -- the three stages and the complex system on waves of their own; 2 a pair of waves per column -- stages and
   real system on one, complex system on the other; same arguments, bit-identical results; -1, the default: chosen per
   context where all waves fit the chip at once -- teams up to 128 columns, pairs up to 512, nk2d_team_auto),
   "pc_valu" (1: the round-1 preconditioner kernels, for A/B runs), "pc_fused" (1, default: from blocks of 1024 rows a panel
   step of the preconditioner's Gauss-Jordan inversions is ONE launch whose first workgroup also inverts the NEXT step's
   pivot block; 2: at every size; 0: the two launches of rounds 1 - 3 -- the same bits either way), "sweep_wpb",
   (closed experiments removed in round 4: "xcd_map", "prefactor" -- profiles/r03_prefactor holds their measurements),
   "frozen_err_check" (k: SciPy's error estimate on every k-th step of a frozen year, default 128; 0 off),
   "frozen_persistent" / "frozen_persistent_max_e" / "frozen_cache_gb" (the one-launch frozen year, see nk2d_get_counter),
   "frozen_team" (1, default: a four-wave team per column inside that launch up to two levels per lane; 0: a wave per
   column), "frozen_wpb" (columns per workgroup of the wave-per-column
   flavour with that hand-over, 1 .. 4, default 2: the waves of a workgroup move in lock step, a neighbour in another
   workgroup is read over the fabric), "frozen_coef_lds" (bits, default 63: what a wave of that flavour keeps on its compute unit
   for the year at three and more levels per lane -- 1 the static coefficients of its column, 2 W, 4 the step's mixing columns and
   vertical Jacobian diagonals, 8 the real system's pivots, 16 the column's own state Y, all of them in LDS, and 32 the column's
   own three stage values in registers from one Newton phase to the next; bits 4 and 8 need "frozen_by_column"; bits 16 and 32
   exist on top of the other four, on the full cache, at five to seven levels per lane -- a cache in pieces has 32 only together
   with 16 --; what does not fit the compute unit's LDS is given up, 16 first: counter "frozen_lds_bits" is the set the year
   launched last ran with), "frozen_early" (1, default, or 0: a wave that carries the whole own state -- "frozen_lds_bits" 63 --
   forms the norm partial of an update part behind that part's stores, while they are on their way, and stores it behind its
   hand-over flag instead of in front of the stores its neighbours wait for; the same operations; counter "frozen_early_bits"),
   "frozen_stage_exchange" (1, default, or 0: the waves that carry the whole own state publish the stage values U_i = Y + Z_i of
   their column in place of Z_i, and a stage part takes its neighbours' three columns from there with no load of their Y and no
   addition, its own from its registers: 14 of a stage phase's 56 loads over the fabric go; the same operands in the same
   addition, on the producing side: the same bits; Z goes to memory only in the rows with an error estimate and in the last;
   not on a cache in pieces with linear sources at seven levels per lane, which stays on the body without it;
   counter "frozen_stage_exchange_bits"),
   "frozen_xlane" (1 or 0: on top of the stage-value exchange, the Newton phase moves values between lanes -- the vertical stencil
   of the tendencies, the parallel cyclic reduction of the two tridiagonal solves, the sum of the norm partial -- with DPP and
   v_permlane swaps in the VALU instead of ds_bpermute through LDS; every lane receives the same 64 bits: the same year bit for
   bit; no decision, not part of the schedule fingerprint; counter "frozen_xlane_bits"),
   "frozen_dedicated" (0, 1 or 2, anything else is an error; default 2; read at every frozen year: a year that would run the Newton
   body of every default -- all of the column in LDS and registers, "frozen_early", the stage-value exchange and the VALU moves in
   effect: linear sources at five to seven levels per lane on the full cache, "frozen_lds_bits" 63 -- runs in k_frozen_persistent_d, the
   same kernel text compiled with that one body instead of twenty and with what the host guarantees for it as constants; 2: and
   its hand-over polls the two neighbours' flags and the abort flag with one load per spin; the same device functions: the same
   year bit for bit; no decision, not part of the schedule fingerprint or the cache key; counters "frozen_dedicated_bits",
   "frozen_dedicated_years"),
   "xlane_selftest_in0" .. "xlane_selftest_in63" and "xlane_selftest_run" (the self-test of those moves, no entry point of its own:
   the 64 doubles of one wave, lane by lane, then 1 to run it: one wave moves them -- as a complex value too: that vector and
   the same vector read backwards -- by 1, 2, 4, 8, 16 and 32 lanes; counter "xlane_selftest_<w>_<row>_<lane>" is then the 64 bits
   lane <lane> holds of row <row>, as __shfl_up / __shfl_down give them (w = 0) and as the VALU helper gives them (w = 1); rows
   0-5 up, 6-11 down, 12-17 / 18-23 complex up (re / im), 24-29 / 30-35 complex down, 36 the sum over the wave, of which only
   lane 0 holds the total),
   "frozen_sums_poison" (0, default, or 1; for tests: the rows of norm partials are filled with NaN before every frozen year, so
   that a partial the year does not store fails its check instead of passing on what an earlier year left there),
   "frozen_by_column" (1,
   default: from five levels per lane a workgroup is ONE ypos column with all its tracers, so that what is the same for every
   tracer of a column is shared through LDS; 2: from three levels per lane; 0: adjacent columns of one tracer),
   "hook_spec_depth" (1 or 2, default 2: whole Newton iterations a controller with a vector norm hook queues ahead of a verdict), "barrier_timeout_ms" (longest wait at a grid barrier of the one-launch years, default 2000:
   then the year is rerun launch by launch), "year_fences" (1: release / acquire fences around those barriers, validation),
   "pc_fp32" (1: the preconditioner's Schur inverses stored in single precision -- half the HBM -- and every apply refined
   "pc_refine" times, default 1, against the exact block tridiagonal operator; set before nk2d_precond_setup),
   "pc_two_ended" (0, default, or 1; opt-in: the preconditioner's block elimination runs from ypos = 0 and ypos = ny - 1 at
   once -- two chains of half the length in the same launches, a twisted factorisation -- and meets in column ny / 2, and
   the substitution advances both chains per launch.  Read by nk2d_precond_setup, nk2d_precond_setup_states and
   nk2d_shift_factor; nk2d_precond_apply and nk2d_shift_solve follow the value of the set-up they use.  Composes with
   "pc_fp32" and "pc_fused"; with "pc_valu" 1 the set-up is refused.  Counters "pc_setup_rounds", "pc_sub_launches"),
   "pc_pivot_wave" (0, default, or 1; opt-in: the 32 x 32 pivot blocks of the preconditioner's Gauss-Jordan inversions are
   inverted by ONE wave in registers -- no LDS round trip and no barrier per pivot -- instead of by four waves through LDS:
   the same operations in the same order, the same bits.  Read at every set-up as "pc_two_ended" is; composes with
   "pc_fused", "pc_valu", "pc_two_ended" and "pc_fp32".  Counter "pc_pivot_wave_steps"),
   "pc_panel" (32, default, or 64; any other value is refused and the value stays.  Opt-in: the preconditioner's Gauss-Jordan
   inversions advance by panels of 64 pivots -- one launch per panel step at every block size, the matrix streamed once per
   64 pivots, a rank-64 update on the matrix cores, the 64 x 64 pivot blocks inverted by four waves in LDS one pivot after
   the other -- instead of 32.  The same pivots in the same order, other rounding between them: held to the references of
   the 32-wide path at its bars, not to its bits.  Read at every set-up as "pc_two_ended" is; "pc_fused" is not consulted;
   composes with "pc_two_ended" and "pc_fp32"; with "pc_valu" 1 or "pc_pivot_wave" 1 the set-up is refused.  The layout of
   the stored inverses is that of 32: a factorisation made with 64 is applied whatever the value is by then.  Counter
   "pc_panel_steps") */
int nk2d_set_option(nk2d_ctx* ctx, const char* name, double value);

/* block until every operation queued on the context's stream has finished */
int nk2d_sync(nk2d_ctx* ctx);
/* the context's HIP stream (hipStream_t as void*), for event timing by the caller */
void* nk2d_stream(nk2d_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* NK2D_H */
