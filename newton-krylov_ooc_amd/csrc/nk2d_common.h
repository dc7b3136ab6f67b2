// nk2d_common.h -- context, device layout and wave-level primitives shared by the
// translation units of libnk2d.so (gfx950 only).
//
// Device layout ("lane-blocked columns").  A state vector of one tracer module is
// [tc][ny] columns; a column holds the nz depth levels of one (tracer, ypos) pair and
// is owned by ONE 64-lane wavefront.  With E = ceil(nz/64) levels per lane, level
// k = lane*E + e is stored at
//
//        ((tr*ny + j)*E + e)*64 + lane
//
// so that (a) every load/store of a column is a fully coalesced 512-byte row per e,
// (b) the vertical neighbours k-1 / k+1 are in the lane's own registers or one DPP
// shuffle away, which is what the vertical-mixing stencil and the per-column
// tridiagonal solves need, and (c) the horizontal neighbours (j-1, j+1) are the same
// (e, lane) slot of the adjacent column.  Levels k >= nz are padding and hold 0.
// Host arrays (C order (tracer, depth, ypos)) are converted at upload / download.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/nk2d.h"

#define NK2D_WAVE 64
#define NK2D_WAVES_PER_BLOCK 4
#define NK2D_BLOCK (NK2D_WAVE * NK2D_WAVES_PER_BLOCK)
#define NK2D_MAX_E 8
#define NK2D_OWN_REC_CAP 65536   /* rows of the context's own schedule record */
#define NK2D_CKPT_EVERY 128      /* steps between two checkpoints of a frozen year */


// option "frozen_early" as a context starts with it (1: the norm partial of an update part behind its stores and the hand-over's flag)
#define NK2D_FROZEN_EARLY_DEFAULT 1
// option "frozen_stage_exchange" as a context starts with it (1: the neighbours of the one-launch year exchange stage values, not Z and Y)
#define NK2D_FROZEN_STAGE_EXCHANGE_DEFAULT 1
// option "frozen_xlane" as a context starts with it (1: the cross-lane moves of the one-launch year's Newton phase go through the VALU)
#define NK2D_FROZEN_XLANE_DEFAULT 1
// option "frozen_dedicated" as a context starts with it (0: k_frozen_persistent; 1: the entry that carries the default year's body alone,
// k_frozen_persistent_d; 2: that entry with the hand-over's one-load poll)
#define NK2D_FROZEN_DEDICATED_DEFAULT 2
// ... and which moves that body takes from the xl_ helpers: the sum of the distances (1 | 2 | 4 | 8 | 16 | 32) and NK2D_XL_SUM (64)
#ifndef NK2D_FROZEN_XLANE_MOVES
#define NK2D_FROZEN_XLANE_MOVES 97
#endif
struct nk2d_ctx {
    nk2d_desc d;
    int nz, ny, tc, E, nzp, ncol, nreg;
    int kind;   // module kind: 0 linear sources (iage, forced), 1 phosphorus, 2 forced with forcing files
    size_t nv;  // doubles per state vector  (tc*ny*nzp)
    size_t np;  // doubles per (depth, ypos) plane (ny*nzp)
    int dev;
    hipStream_t stream_;   // the context's stream: through nk2d_s(c), which first ends a running command-stream kernel
    std::string err;
    // the year as a command stream (nk2d_stream.hip): ONE resident kernel executes the launches of the host-controlled year
    // as commands, workgroups handing over to their lateral neighbours instead of meeting at launch boundaries
    struct nk2d_stream_state* strm;
    int stream_years;      // option "stream_years": 1 = forward years of eligible contexts run as command streams
    int stream_two_waves;  // option "stream_two_waves": the 256-register flavour of the kernel where it lets every column be resident
    int stream_xlane;      // option "stream_xlane": the resident kernel's cross-lane moves at distances 1 and 32 and its wave sums in the VALU
    int stream_xlane_bits; // counter "stream_xlane_bits": what the resident kernel launched last ran with
    int stream_on;         // set by the integrator for the span of a year that may run as a command stream
    int stream_lost;       // years in a row whose kernel gave up (two: the context stops trying)
    int64_t stream_cmds, stream_launches, stream_timeouts, stream_years_run;   // counters (nk2d_get_counter)
    // a frozen year replayed from a command tape in HBM (option "frozen_tape", nk2d_stream.h): recorded once per schedule
    // (tape_rec: nk2d_stream_push appends to the tape, nothing runs; tape_foreign counts launches that have no command)
    int frozen_tape;
    struct nk2d_tape* tape;
    int tape_rec, tape_foreign;
    int64_t tape_years_run, tape_builds, tape_timeouts;   // counters (nk2d_get_counter)
    int64_t tape_fallbacks;   // ... and taped years handed to the existing path without a timeout (not resident, refused recording)

    // static, packed planes (device)
    double* VV;      // vvel at ypos faces, (ny+1) columns
    double* KH;      // horizontal mixing coeff at ypos faces, (ny+1) columns, walls 0
    double* WT;      // wvel at the top face of cell k,    ny columns
    double* WB;      // wvel at the bottom face of cell k, ny columns
    double* DZR;     // depth.delta_r           [nzp]
    double* ZM0;     // depth.mid[k]            [nzp]
    double* ZM1;     // depth.mid[k+1]          [nzp]
    double* DM;      // depth.delta_mid[k]      [nzp]
    double* DMR;     // depth.delta_mid_r[k]    [nzp]
    double* DYR;     // ypos.delta_r            [ny]
    double* BLDMAX;  // bldepth_max             [ny]
    // region data
    int32_t* MASK;   // [np]
    double* WN;      // grid_weight / sum over region [np]
    // Jacobian planes at t_jac (tracer independent part), np each
    double *JL, *JU, *JS, *JN, *JC;
    // phosphorus module: light limitation [np], d uptake / d po4 at the linearisation state [np],
    // linearisation state of the stand-alone Jacobian entry points [nv]
    double *LIGHT, *UPR, *YLIN;
    // kind 2: forcing records on the device (packed planes / rows), their times on the host, and the length
    // of a KV buffer: the vertical mixing plane, then (kind 2) the source plane and the restoring targets of
    // the same time -- whatever is a function of time alone travels in one bundle
    double *SMSREC, *RESTREC;
    double *sms_t, *rest_t;
    size_t kv_len;
    int ylin_set;
    // vertical mixing planes: 3 stage times, current t, scratch
    double* KV[5];
    // second sets: the launch that ends a frozen step writes the next attempt's stage planes and Jacobian planes while
    // its own stage and sweep parts still read the current ones (nk2d_r_newton_final)
    double* KVN[3];
    double* JB[5];
    // Radau work vectors (nv each unless noted)
    double *Y, *YOLD, *F, *Z /*3nv*/, *ZP /*3nv*/, *W /*3nv*/;
    // third stage buffer: a simplified-Newton iteration whose solve needs ONE sweep runs as a single launch
    // (stage + sweep + update); its update writes the new stage values here while the neighbouring columns still read
    // the old ones from Z in the same launch, then Z and ZN swap
    double* ZN /*3nv*/;
    int min_sweeps;    // least sweeps per solve where columns couple (option "min_sweeps": 1 default, 2 = round-1 rule)
    std::vector<double> last_sched;     // accepted steps of the most recent free-running year (nk2d_last_schedule)
    std::vector<double> own_rec;        // its record buffer when the caller gave none
    std::vector<double> frozen_sched;   // accepted steps the perturbed years of nk2d_jvp repeat (nk2d_set_frozen_schedule)
    int jac_stage_state;   // 1: option "jac_stage" also for modules whose Jacobian reads the state (plane of the stage time, state of the step start)
    int final_fuse;    // 1: a frozen step ends in the launch of its last Newton iteration (option "final_fuse", for A/B runs)
    int jac_stage;     // >= 0: Jacobian of a step attempt from the vertical mixing plane of this stage time (option "jac_stage"); -1: step start
    int team;          // 1: Newton-iteration launches run as k_newton_team (one workgroup per column); 0: k_newton_fused (option "team")
    int single_swap;   // 1: single-launch iterations write ZN and swap (host-side decisions; see nk2d_radau.hip set_lu)
    int swap_updates;  // 1: ... and so do the update launches of several-sweep iterations (vector norm hook)
    double *BR, *BCR, *BCI, *XR[2], *XCR[2], *XCI[2], *TMP, *TMP2;
    // cached line factorisation of the current (h_lu, t_jac): pivot reciprocals and PCR tables
    double *FR_INV, *FC_INVR, *FC_INVI;   // nv each
    double *FR_TAB, *FC_TABR, *FC_TABI;   // ncol * NK2D_TAB * 64 each
    // single precision copies for the fused Newton launches: the line factorisation is an approximate
    // inverse inside an iteration that re-evaluates the exact residual, its storage precision only
    // touches the contraction rate (nk2d_set_option "factor_fp32")
    float *FR32_INV, *FC32_INVR, *FC32_INVI, *FR32_TAB, *FC32_TABR, *FC32_TABI;
    int factor_fp32;
    hipEvent_t snap_ev[8];  // "the launch that carries these partials is queued" (host-side decisions by launches)
    int snap_ready;
    int sweep_wpb;          // waves per block of the sweep kernel (1, 2 or 4)
    int jac_fresh;          // 1: re-evaluate the Jacobian at every step start (see nk2d_set_option)
    double growth_cap;      // > 0: largest step growth factor after a step whose Newton iteration failed at first
                            // (nk2d_set_option "growth_cap"; 0 = SciPy: no memory of the failure)
    // reductions
    double* PART;    // per-task partials
    double* PART2;   // second buffer [ncol]
    double* STEP_PART;      // frozen year: norm partials of the last two Newton iterations of every step, rows of ncol
    size_t step_part_rows;  // rows allocated
    double* STEP_NORM;  // [3 * NK2D_OWN_REC_CAP] per step of a frozen year: sum((dW/scale)^2) of its last and last-but-one iteration, sum((err/scale)^2)
    // frozen years given up with -7: rejected by the a-posteriori Newton check or by a sampled error estimate (nk2d_frozen_fallbacks).
    // For module_kind 1 ALSO the one-launch years of option "frozen_phosphorus" that a hand-over time-out handed back to the
    // launch-per-phase path, which then reran them (run_replay; for the other modules such a hand-back shows in nbarrier_timeouts only)
    int64_t frozen_fallbacks;
    // the frozen year of a small grid in one launch on a schedule cache (k_frozen_persistent, nk2d_kernels.hip)
    void* frozen_cache;
    int frozen_persistent;          // option "frozen_persistent": 1 = where eligible (default), 0 = never
    int frozen_persistent_max_e;    // ... for grids of at most this many levels per lane (option "frozen_persistent_max_e")
    double frozen_cache_max_gb;     // ... whose schedule cache stays below this size (option "frozen_cache_gb")
    int64_t frozen_cache_builds, frozen_persistent_years;
    int frozen_team;      // option "frozen_team": a four-wave team per column inside the one-launch frozen year (grids of at most two levels per lane)
    int frozen_wpb;       // option "frozen_wpb": columns (waves) per workgroup of the wave-per-column one-launch year with neighbour hand-over
    int frozen_coef_lds;  // option "frozen_coef_lds": the one-launch year keeps the static coefficients of a wave's column in LDS
    int frozen_lds_bits;  // counter "frozen_lds_bits": the bits of it in effect in the one-launch year launched last, after fitting
    int frozen_early;     // option "frozen_early": a wave of the one-launch year forms its norm partials out of the way of the hand-over
    int frozen_early_bits; // counter "frozen_early_bits": the option in effect in the one-launch year launched last
    int frozen_stage_exchange;      // option "frozen_stage_exchange": the neighbours of the one-launch year exchange the stage values Y + Z_i, not Z_i and Y
    int frozen_stage_exchange_bits; // counter "frozen_stage_exchange_bits": the option in effect in the one-launch year launched last
    int frozen_xlane;               // option "frozen_xlane": the Newton phase of the one-launch year moves values between lanes in the VALU, not through LDS
    int frozen_xlane_bits;          // counter "frozen_xlane_bits": the option in effect in the one-launch year launched last
    int frozen_dedicated;           // option "frozen_dedicated": 1, 2 the one-launch year in the entry with the default year's body alone (2: one-load poll)
    int frozen_dedicated_bits;      // counter "frozen_dedicated_bits": the option in effect in the one-launch year launched last (frozen_dedicated())
    int64_t frozen_dedicated_years; // counter "frozen_dedicated_years": one-launch years that entry ran (also counted in frozen_persistent_years)
    int frozen_by_column; // option "frozen_by_column": a workgroup of the one-launch year is one ypos column with all its tracers
    int frozen_alloc_async;   // option "frozen_alloc_async": a schedule cache above 8 GB is allocated by a thread of its own
    int frozen_cache_after;   // option "frozen_cache_after": frozen years of a schedule that run launch by launch before its cache is built (default 0; -1: 0 for a cache below 8 GB, 3 above)
    // option "frozen_cache_pieces": the schedule cache as a list of equally sized pieces (one hipMalloc each) instead of one slab
    int frozen_cache_pieces;          // 0 (default): the slab, 1: pieces
    double frozen_cache_piece_mb;     // option "frozen_cache_piece_mb": size of a piece in MiB (rows per piece = floor of it over a row's bytes, at least 1)
    int64_t frozen_cache_piece_rows;  // option "frozen_cache_piece_rows": rows per piece directly (0: from the size in MiB)
    // option "frozen_cache_lean": the schedule cache holds the planes only, the one-launch year factorises in the first phase of every step
    int frozen_cache_lean;            // 0 (default): the full cache, 1: lean, 2: lean where the full cache would be refused
    int64_t frozen_lean_years;        // lean one-launch years run (also counted in frozen_persistent_years)
    uint64_t frozen_lean_mem_key;     // mode 2: the schedule whose full cache the 85 % rule refused last
    // option "frozen_forced": the one-launch year for the file-driven forced module (kind 2) where it has none by default
    int frozen_forced;                // bit mask, default 0.  1: linear sources at five to eight levels per lane; 2: a thresholded sink (lean cache only)
    int64_t frozen_forced_years;      // one-launch years only that option made possible (also counted in frozen_persistent_years)
    // option "frozen_phosphorus": the one-launch year for the phosphorus module (kind 1), on the lean cache, three to eight levels per lane
    int frozen_phosphorus;            // default 0.  1: one wave per SIMD; 2: the 256-register flavour where that one is not resident; 3: it wherever it exists
    // option "frozen_phosphorus_shallow": ... and at one and two levels per lane (the same by-column workgroup, nothing of the year in LDS)
    int frozen_phosphorus_shallow;    // default 0, or 1
    int64_t frozen_phosphorus_shallow_years;   // one-launch years only that option made possible (also counted in frozen_phosphorus_years)
    int frozen_two_waves_last;        // 1: the one-launch year just run was the 256-register flavour (k_frozen_persistent_w2)
    int64_t frozen_phosphorus_years;  // one-launch years of that module (also counted in frozen_persistent_years and frozen_lean_years)
    int64_t frozen_two_waves_years;   // of them: the years that ran the 256-register flavour
    int frozen_cache_early;           // option "frozen_cache_early": with pieces, the year that records a schedule asks for its pieces when it ends
    int64_t frozen_cache_piece_allocs, frozen_cache_early_requests;   // counters: pieces allocated so far, early requests made
    uint64_t frozen_seen_key; int frozen_seen_years;   // the schedule last seen by nk2d_frozen_persistent and its years so far
    int64_t frozen_team_years;
    int64_t frozen_launch_us;   // device time of the one-launch frozen years so far (HIP events around the launch)
    double barrier_timeout_ms;  // longest wait at a grid barrier of the persistent year (option "barrier_timeout_ms")
    int year_fences;            // 1: release / acquire fences around its grid barriers (option "year_fences", validation)
    int64_t frozen_resumes;     // ... and resumed from a checkpoint with one more Newton iteration (nk2d_frozen_resumes)
    int frozen_err_check;       // k > 0: SciPy's error estimate on every k-th step of a frozen year (option "frozen_err_check")
    uint64_t grid_hash;         // hash of the grid / module description given to nk2d_create (nk2d_fingerprint)
    // state kept every NK2D_CKPT_EVERY steps of a frozen year (Y, YOLD, ZP: 5 nv doubles each) for the resume
    std::vector<double*> ckpt;
    double* RED;     // reduced scalars (device)
    double* hRED;    // pinned host mirror
    double* hPART;   // pinned, device-visible per-column partials [ncol] (host-controlled integrator)
    double* hPART2;  // same, for an error estimate queued behind a Newton iteration not yet judged
    double* hPARTB;  // same, second buffer for Newton iterations queued one ahead of the one being judged
    double* hPARTC;  // ... and two ahead (vector norm hook)
    double* ZS /*3nv*/;   // second spare set of stage values, allocated with a vector norm hook: iterations queued TWO ahead
    int hook_spec_depth;  // option "hook_spec_depth": whole iterations a hooked controller queues ahead of a verdict (1 or 2)
    // what the host-side controller queued ahead of a verdict and had to drop (nk2d_get_counter)
    int64_t cnt_spec_dropped, cnt_front_dropped, cnt_err_void, cnt_err_queued;
    double* part_cur;  // where the next fused launch with the update puts its partials (null: hPART / PART)
    int part_on_host;
    int factor_pending;          // set by the integrator's "LU" event, consumed by the next fused launch
    double lu_cre, lu_ccr, lu_cci;  // shifts of the current line factorisation
    int speculate;   // 1: queue the next Newton iteration's front launches before reading the norm
    double spec_bias;   // option "spec_bias": the iteration in flight is EXPECTED to pass SciPy's convergence test when its predicted test value is below this many tolerances (what is queued behind it: the error estimate or another iteration; never a decision)
    // freed state vectors kept for reuse (nk2d_vec_alloc / nk2d_vec_free)
    std::vector<double*> vec_pool;
    std::mutex pool_mutex;
    // staging for host <-> device layout conversion
    double* STAGE;
    double* hSTAGE;  // pinned host twin of STAGE
    size_t stage_elems;
    // downloads in two halves (nk2d_vec_download_begin / _end): staging pairs of their own, kept for reuse
    struct nk2d_download_pool* dl_pool;
    // region scalars staged on device for the algebra kernels
    double* RCOEF;
    double* hRCOEF;  // pinned host twin of RCOEF
    size_t rcoef_elems;

    // line-relaxation contraction bound rho(c) = max_i s_i / (c + q_i), tabulated at create
    // on a log grid of shifts c (rho is decreasing in c: the entry at the grid point below c
    // is a valid, at most ~4 % pessimistic bound)
    std::vector<double> rho_tab;
    double rho_c0, rho_dlog;   // first grid shift, log10 spacing
    // preconditioner (banded LU), see nk2d_precond.hip
    void* precond;
    int pc_fused;  // 1 (default): a panel step of the Gauss-Jordan inversions is ONE launch (k_pc_gj_step) for blocks of 1024 rows and more; 2: at every size; 0: two launches (k_pc_gj_rows + k_pc_gj_update_mfma) -- the same bits
    int pc_valu;   // 1: the round-1 preconditioner kernels (VALU rank-32 update, 8-byte mat-vec loads), for A/B runs
    int pc_fp32;   // 1: Schur inverses of the linear modules' preconditioner stored in single precision (option "pc_fp32")
    int pc_refine; // ... with this many refinement steps per apply against the exact operator (option "pc_refine", default 1)
    int pc_two_ended;   // option "pc_two_ended": 0 (default) the block elimination runs over ypos = 0 .. ny - 1, 1 from both ends at once (read at set-up; a factorisation keeps the value it was made with)
    int64_t pc_setup_rounds, pc_sub_launches;   // counters (nk2d_get_counter): dependent inversion rounds of the last elimination, dependent mat-vec launches of the last substitution
    int pc_pivot_wave;  // option "pc_pivot_wave": 0 (default) the 32 x 32 pivot blocks of the Gauss-Jordan inversions are inverted by four waves through LDS, 1 by one wave in registers -- the same bits (read at every set-up)
    int64_t pc_pivot_wave_steps;   // counter: panel steps of the last elimination that ran a wave flavour
    int pc_panel;  // option "pc_panel": 32 (default) or 64 pivots per panel step of the Gauss-Jordan inversions; 64 is the one-launch step k_pc_gj_step64 at every size, pc_fused is not consulted (read at every set-up)
    int64_t pc_panel_steps;   // counter: 64-wide panel steps of the last elimination
    int64_t pc_phos_applies;  // counter: nk2d_precond_apply calls of this context that ran the one-call phosphorus preconditioner (null-vector form of nk2d_precond_setup_states)

    // optional dense-output sampling of the running comp_fcn (history files)
    int hist_n, hist_next;
    const double* hist_t;
    double* hist_host;   // [hist_n][tc][nz][ny]
    // ... as commands of the year's resident kernel (option "stream_hist", nk2d_stream.h: NK2D_OP_DENSE_OUT): packed samples
    // wait in the slots of a buffer in HBM until the kernel has ended (the slots are full; the end of the year)
    int stream_hist;             // option "stream_hist": 0 (default) a sampled step is a piece of launches, 1 its samples are commands
    double stream_hist_mb;       // option "stream_hist_mb": budget of the sample buffer in MiB (0: one slot)
    double* HISTBUF;             // [hist_slots][nv]
    size_t hist_slots, hist_buf_elems;   // slots of this year, doubles allocated
    std::vector<int> hist_slot_k;        // the sample each filled slot holds, in the order they were filled
    int64_t hist_year_samples, hist_year_drains;   // what the running year has drained so far: booked when the year stands
    int64_t stream_hist_samples, stream_hist_drains;   // counters (nk2d_get_counter): years that ran as streams to their end

    // counters of the running comp_fcn
    nk2d_stats st;

    // coupling of the integrator's scalar norms across contexts that share one tracer module (tracers
    // sharded over GPUs, nk2d_set_norm_hook): every sum of squares the controller reads goes through
    // norm_hook (an all-reduce supplied by the caller) and n_total is the module's size, not the shard's
    nk2d_norm_hook_fn norm_hook;
    void* norm_hook_user;
    nk2d_norm_hook_vec_fn norm_hook_vec;   // several sums per call (nk2d_set_norm_hook_vec); norm_hook then wraps it
    void* norm_hook_vec_user;
    double global_n;
    // persistent whole-year kernel (device_ctl 3, nk2d_kernels.hip): norm partials [2][ncol], result block,
    // barrier counter + abort flag, sweeps-per-shift table, schedule record, timing events
    double *YR_PART, *YR_OUT, *hYR_OUT, *YR_REC;
    void* YR_SYNC;
    int* YR_MTAB;
    double yr_lin_tol;
    int64_t yr_rec_cap;
    hipEvent_t yr_ev[2];
    // generic event pair on the context's stream (nk2d_timer_begin / nk2d_timer_end)
    hipEvent_t timer_ev[2];
    int timer_ready;

    // sampled HIP-event timing of the line-relaxation sweep kernel (nk2d_profile_*)
    int prof_every;
    std::vector<hipEvent_t> prof_ev;  // start/stop pairs
    size_t prof_used;                 // events in use (2 per sample)
    double prof_ms_sum;
    double prof_overhead_ms;          // elapsed time of an EMPTY event pair (calibration)
    int64_t prof_cnt;
    int64_t sweep_launches;           // launches of the dominant kernel since the last nk2d_profile_reset
    double fused_bytes_all;           // algorithmic bytes of ALL those launches (timed or not)
    int64_t shape_cnt[4];             // non-factorising launches by shape: stage+update, stage only, update only, neither
    double shape_bytes[4];            // their algorithmic bytes
    double sweep_bytes;               // algorithmic bytes of the launches inside timed windows
    int64_t prof_windows;             // timed windows folded into prof_ms_sum (prof_cnt: their launches)
    std::vector<int> prof_win_launches;
    int win_open, win_launches;
    int64_t win_seq;
    double win_bytes;
    // the check behind a frozen year, made observable (tests): option "frozen_sums_poison" fills the rows of STEP_PART with NaN
    // before every frozen year -- a partial that is not stored, or stored elsewhere, then fails the year's check instead of
    // passing on what the year before left there --; counter "frozen_step_sums_hash" is a 64-bit FNV-1a hash of the bits of
    // the step sums the last whole-year check read (last iteration of every step, and the one before where there is one)
    int frozen_sums_poison = 0;
    int64_t frozen_step_sums_hash = 0;
};

#define NK2D_CHECK(ctx, call)                                                        \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_) + " at " + \
                         __FILE__ + ":" + std::to_string(__LINE__);                  \
            return -1;                                                               \
        }                                                                            \
    } while (0)

#define NK2D_TRY(expr)            \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

// nk2d_stream.hip (the year as a command stream, nk2d_stream.h)
void nk2d_turn_take(int waves);   // resident kernels of a process: one at a time, or side by side where their waves leave room
void nk2d_turn_give(int waves);
#define NK2D_RC_STREAM_LOST 17   /* the command-stream kernel gave up (a wait timed out): the caller reruns the year by launches */
int nk2d_stream_pause(nk2d_ctx* c);
bool nk2d_stream_running(const nk2d_ctx* c);
int nk2d_stream_columns_per_workgroup(const nk2d_ctx* c);
int nk2d_stream_two_waves(const nk2d_ctx* c);
int nk2d_stream_eligible(const nk2d_ctx* c);
int nk2d_stream_ready(nk2d_ctx* c);     // buffers of the command stream in place (first use)
int nk2d_stream_end(nk2d_ctx* c);       // ends the kernel, waits for it; NK2D_RC_STREAM_LOST if it had given up on the way
void nk2d_stream_free(nk2d_ctx* c);
int64_t nk2d_tape_size(const nk2d_ctx* c, int what);   // the current tape: 0 bytes, 1 commands
void nk2d_tape_forget(nk2d_ctx* c);   // a buffer a recorded command may point at is reallocated: the tape is recorded again
int nk2d_stream_profile(nk2d_ctx* c, double* out12);
double* nk2d_stream_part_take(nk2d_ctx* c, const double* name);
const double* nk2d_stream_part_named(const nk2d_ctx* c, const double* name);
void nk2d_stream_part_forget(nk2d_ctx* c, const double* name);
int nk2d_stream_wait_part(nk2d_ctx* c, const double* part, int n);
// the stream every launch, copy and synchronisation of a context goes to: whatever is queued there must come AFTER the
// commands pushed so far, so a resident command-stream kernel is told to finish first (the caller's launch is then ordered
// behind it by the stream; nothing is waited for here)
static inline hipStream_t nk2d_s(nk2d_ctx* c) {
    if (c->tape_rec) c->tape_foreign++;     // (recording a tape: this launch would run now, not in its place on the tape)
    if (c->strm && nk2d_stream_running(c)) (void)nk2d_stream_pause(c);
    return c->stream_;
}

static inline int nk2d_fail(nk2d_ctx* c, const std::string& msg, int code = -2) {
    c->err = msg;
    return code;
}

// Launch shape of the Newton-iteration launches by default: 0 one wave per column (k_newton_fused), 1 a team of four waves
// (k_newton_team), 2 a pair of waves (k_newton_pair).  All three give bit-identical results.  A team or pair wave holds
// at most 256 VGPRs, so the chip's 1024 SIMDs take 2048 of them at once; beyond that the workgroups run in rounds and
// the split loses (iage 416^2, 832 columns: 22.5 us per launch with teams, frozen year 0.225 s with pairs, against
// 16.4 us / 0.198 s with one wave per column).  Where everything is resident it wins, the more the smaller the grid --
// frozen year of iage, one wave / team / pair per column: 26^2 18.6 / 15.9 / 16.0 ms, 52^2 30.0 / 25.7 / 26.0 ms,
// 104^2 54.1 / 48.1 / 46.4 ms, 208^2 97.9 / 98.3 / 93.7 ms; one-tracer module at 416^2 (416 columns of 7 levels per
// lane): year 0.66 -> 0.60 s with teams (profiles/r02_team*.log).
static inline int nk2d_team_auto(const nk2d_ctx* c) {
    if (c->ncol <= 128) return 1;
    if (c->ncol <= 512) return (c->E >= 5) ? 1 : 2;
    return 0;
}

static inline int nk2d_grid(int ntasks) { return (ntasks + NK2D_WAVES_PER_BLOCK - 1) / NK2D_WAVES_PER_BLOCK; }

// run `stmt` with a compile-time constant EE equal to the runtime levels-per-lane
#define NK2D_DISPATCH_E(Eval, ...)                                 \
    switch (Eval) {                                                  \
        case 1: { constexpr int EE = 1; __VA_ARGS__; } break;               \
        case 2: { constexpr int EE = 2; __VA_ARGS__; } break;               \
        case 3: { constexpr int EE = 3; __VA_ARGS__; } break;               \
        case 4: { constexpr int EE = 4; __VA_ARGS__; } break;               \
        case 5: { constexpr int EE = 5; __VA_ARGS__; } break;               \
        case 6: { constexpr int EE = 6; __VA_ARGS__; } break;               \
        case 7: { constexpr int EE = 7; __VA_ARGS__; } break;               \
        case 8: { constexpr int EE = 8; __VA_ARGS__; } break;               \
        default: break;                                              \
    }

// the same for the kernels that exist for small grids only (at most 4 levels per lane = 256 depth levels)
#define NK2D_DISPATCH_E4(Eval, ...)                                \
    switch (Eval) {                                                  \
        case 1: { constexpr int EE = 1; __VA_ARGS__; } break;               \
        case 2: { constexpr int EE = 2; __VA_ARGS__; } break;               \
        case 3: { constexpr int EE = 3; __VA_ARGS__; } break;               \
        case 4: { constexpr int EE = 4; __VA_ARGS__; } break;               \
        default: break;                                              \
    }

// as above, plus a compile-time module kind KK (0: linear sources, 1: phosphorus, 2: forcing files)
#define NK2D_DISPATCH_EK(Eval, kind, ...)                                        \
    if ((kind) == 1) {                                                            \
        constexpr int KK = 1;                                                     \
        NK2D_DISPATCH_E(Eval, __VA_ARGS__)                                        \
    } else if ((kind) == 2) {                                                     \
        constexpr int KK = 2;                                                     \
        NK2D_DISPATCH_E(Eval, __VA_ARGS__)                                        \
    } else {                                                                      \
        constexpr int KK = 0;                                                     \
        NK2D_DISPATCH_E(Eval, __VA_ARGS__)                                        \
    }

// ---------------------------------------------------------------------------------
// device primitives
// ---------------------------------------------------------------------------------
#ifdef __HIPCC__

struct cplx {
    double re, im;
};
__device__ __forceinline__ cplx c_make(double r, double i) { cplx z; z.re = r; z.im = i; return z; }

// arithmetic helpers overloaded for double / cplx so the solver template serves both
__device__ __forceinline__ double t_from_real(double a, double) { return a; }
__device__ __forceinline__ cplx t_from_real(double a, cplx) { return c_make(a, 0.0); }
__device__ __forceinline__ double t_zero(double) { return 0.0; }
__device__ __forceinline__ cplx t_zero(cplx) { return c_make(0.0, 0.0); }
__device__ __forceinline__ double t_one(double) { return 1.0; }
__device__ __forceinline__ cplx t_one(cplx) { return c_make(1.0, 0.0); }

__device__ __forceinline__ double t_neg(double a) { return -a; }
__device__ __forceinline__ cplx t_neg(cplx a) { return c_make(-a.re, -a.im); }
__device__ __forceinline__ double t_mul(double a, double b) { return a * b; }
__device__ __forceinline__ cplx t_mul(cplx a, cplx b) {
    return c_make(__builtin_fma(a.re, b.re, -(a.im * b.im)), __builtin_fma(a.re, b.im, a.im * b.re));
}
__device__ __forceinline__ double t_mulr(double a, double s) { return a * s; }
__device__ __forceinline__ cplx t_mulr(cplx a, double s) { return c_make(a.re * s, a.im * s); }
// a - b*c
__device__ __forceinline__ double t_nfma(double a, double b, double c) { return __builtin_fma(-b, c, a); }
__device__ __forceinline__ cplx t_nfma(cplx a, cplx b, cplx c) {
    double re = __builtin_fma(-b.re, c.re, a.re);
    re = __builtin_fma(b.im, c.im, re);
    double im = __builtin_fma(-b.re, c.im, a.im);
    im = __builtin_fma(-b.im, c.re, im);
    return c_make(re, im);
}
// a - b*s with s real
__device__ __forceinline__ double t_nfmar(double a, double b, double s) { return __builtin_fma(-b, s, a); }
__device__ __forceinline__ cplx t_nfmar(cplx a, cplx b, double s) {
    return c_make(__builtin_fma(-b.re, s, a.re), __builtin_fma(-b.im, s, a.im));
}
// reciprocal for the pivots of diagonally dominant systems (finite, far from 0 and inf):
// hardware estimate + two Newton steps, ~1 ulp, a third of the instructions of an IEEE divide
__device__ __forceinline__ double fast_rcp(double a) {
#ifdef NK2D_IEEE_DIV
    return 1.0 / a;
#else
    double r = __builtin_amdgcn_rcp(a);
    r = __builtin_fma(__builtin_fma(-a, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-a, r, 1.0), r, r);
    return r;
#endif
}
__device__ __forceinline__ double t_recip(double a) { return fast_rcp(a); }
__device__ __forceinline__ cplx t_recip(cplx a) {
    double n = fast_rcp(__builtin_fma(a.re, a.re, a.im * a.im));
    return c_make(a.re * n, -a.im * n);
}

__device__ __forceinline__ double shfl_up_t(double v, int s) { return __shfl_up(v, s, 64); }
__device__ __forceinline__ cplx shfl_up_t(cplx v, int s) { return c_make(__shfl_up(v.re, s, 64), __shfl_up(v.im, s, 64)); }
__device__ __forceinline__ double shfl_down_t(double v, int s) { return __shfl_down(v, s, 64); }
__device__ __forceinline__ cplx shfl_down_t(cplx v, int s) { return c_make(__shfl_down(v.re, s, 64), __shfl_down(v.im, s, 64)); }

// sum over the 64 lanes in a fixed tree order; the total is valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------
// The same moves in the VALU (option "frozen_xlane" of the one-launch year).  __shfl_up / __shfl_down with a constant distance
// compile to one ds_bpermute_b32 per 32-bit half plus the VALU that forms its lane index: LDS-pipeline instructions that return
// in order behind the wave's own LDS reads and share the compute unit's one LDS pipeline.  gfx950 moves lanes in the VALU too:
// DPP on v_mov_b32 (wave_shr:1 / wave_shl:1 across the wave; row_shr / row_shl / row_ror inside a row of 16 lanes, with row and
// bank masks that leave `old` in the lanes they disable) and v_permlane16_swap / v_permlane32_swap.  No lane index, no lgkmcnt.
// Builtins only: the compiler inserts the wait states these reads need behind a VALU write.
// Contract: xl_up<S>(v) / xl_down<S>(v) hold in EVERY lane the 64 bits __shfl_up(v, S, 64) / __shfl_down(v, S, 64) hold there --
// the lane's own value where it has no partner (the PCR multiplies that slot by a zero: another value there could turn the
// sign of a zero or make a NaN).  S is 1, 2, 4, 8, 16 or 32.
//   S = 1      wave_shr:1 / wave_shl:1, bound_ctrl off, old = the value: 1 move per half
//   S = 32     permlane32_swap(v, v): its two results are the two directions: 1 move per half for both
//   S = 16     permlane16_swap(v, v) = rows (0 0 2 2), (1 1 3 3); permlane32_swap of those = rows (0 0 1 1), (2 2 3 3); up is
//              (0 0 1 2), down is (1 2 3 3): one select each
//   S = 2,4,8  inside a row row_shr:S / row_shl:S; the S lanes of a row whose partner lies in the row before (after) take it
//              from the S = 16 move of the value, rotated inside its row (row_ror), under a row mask that leaves out the row
//              with no partner and a bank mask that covers those lanes -- that DPP writes first and the row shift, which keeps
//              `old` exactly in the lanes with no source inside the row, second: no select
// ---------------------------------------------------------------------------------
#define NK2D_DPP_ROW_SHL(n) (0x100 + (n))
#define NK2D_DPP_ROW_SHR(n) (0x110 + (n))
#define NK2D_DPP_ROW_ROR(n) (0x120 + (n))
#define NK2D_DPP_WAVE_SHL1 0x130
#define NK2D_DPP_WAVE_SHR1 0x138
__device__ __forceinline__ int xl_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// both directions of one 32-bit half (what a direction does not need the compiler drops)
template <int S>
__device__ __forceinline__ void xl_both32(int x, int& up, int& dn) {
    static_assert(S == 1 || S == 2 || S == 4 || S == 8 || S == 16 || S == 32, "distance of a cross-lane move");
    if constexpr (S == 1) {
        up = __builtin_amdgcn_update_dpp(x, x, NK2D_DPP_WAVE_SHR1, 0xF, 0xF, false);
        dn = __builtin_amdgcn_update_dpp(x, x, NK2D_DPP_WAVE_SHL1, 0xF, 0xF, false);
    } else if constexpr (S == 32) {
        const auto p = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
        up = (int)p[0];
        dn = (int)p[1];
    } else {
        const auto p = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);    // rows (0 0 2 2), (1 1 3 3)
        const auto q = __builtin_amdgcn_permlane32_swap(p[0], p[1], false, false);                  // rows (0 0 1 1), (2 2 3 3)
        const int row = xl_lane() >> 4;
        const int u16 = (int)(row == 2 ? q[0] : p[0]);      // rows (0 0 1 2)
        const int d16 = (int)(row == 1 ? q[1] : p[1]);      // rows (1 2 3 3)
        if constexpr (S == 16) {
            up = u16;
            dn = d16;
        } else {
            // (a bank is four lanes: at S = 2 the mask covers two lanes too many, which the row shift then writes)
            constexpr int lo = S == 8 ? 0x3 : 0x1, hi = S == 8 ? 0xC : 0x8;
            const int tu = __builtin_amdgcn_update_dpp(x, u16, NK2D_DPP_ROW_ROR(S), 0xE, lo, false);
            up = __builtin_amdgcn_update_dpp(tu, x, NK2D_DPP_ROW_SHR(S), 0xF, 0xF, false);
            const int td = __builtin_amdgcn_update_dpp(x, d16, NK2D_DPP_ROW_ROR(16 - S), 0x7, hi, false);
            dn = __builtin_amdgcn_update_dpp(td, x, NK2D_DPP_ROW_SHL(S), 0xF, 0xF, false);
        }
    }
}
template <int S>
__device__ __forceinline__ void xl_both(double v, double& up, double& dn) {
    int ulo, uhi, dlo, dhi;
    xl_both32<S>(__double2loint(v), ulo, dlo);
    xl_both32<S>(__double2hiint(v), uhi, dhi);
    up = __hiloint2double(uhi, ulo);
    dn = __hiloint2double(dhi, dlo);
}
template <int S>
__device__ __forceinline__ double xl_up(double v) { double u, d; xl_both<S>(v, u, d); return u; }
template <int S>
__device__ __forceinline__ double xl_down(double v) { double u, d; xl_both<S>(v, u, d); return d; }
template <int S>
__device__ __forceinline__ cplx xl_up(cplx v) { return c_make(xl_up<S>(v.re), xl_up<S>(v.im)); }
template <int S>
__device__ __forceinline__ cplx xl_down(cplx v) { return c_make(xl_down<S>(v.re), xl_down<S>(v.im)); }

// wave_sum's additions in wave_sum's association; the total is valid in lane 0 -- and only there: each level moves only what
// lane 0's tree reads (lanes 0 .. S-1 take lanes S .. 2S-1), one move per half
template <int S>
__device__ __forceinline__ int xl_fold32(int x) {
    if constexpr (S == 32) return (int)__builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false)[1];
    else if constexpr (S == 16) return (int)__builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false)[1];
    else return __builtin_amdgcn_update_dpp(x, x, NK2D_DPP_ROW_SHL(S), 0xF, 0xF, false);
}
template <int S>
__device__ __forceinline__ double xl_fold(double v) {
    return __hiloint2double(xl_fold32<S>(__double2hiint(v)), xl_fold32<S>(__double2loint(v)));
}
__device__ __forceinline__ double xl_wave_sum(double v) {
    v += xl_fold<32>(v); v += xl_fold<16>(v); v += xl_fold<8>(v);
    v += xl_fold<4>(v); v += xl_fold<2>(v); v += xl_fold<1>(v);
    return v;
}

// The helper family of a body (template parameter XL of tridiag_apply, shift_prev / shift_next, tend_col, norm_partial_sum):
// 0 is __shfl, today's text; otherwise the sum of the distances S that go through the VALU (1, 2, 4, 8, 16, 32: each is its own
// bit), the others staying on ds_bpermute, plus NK2D_XL_SUM for xl_wave_sum.
#define NK2D_XL_SUM 64
template <int XL, int S, typename T>
__device__ __forceinline__ T xl_sel_up(T v) {
    if constexpr ((XL & S) != 0) return xl_up<S>(v);
    else return shfl_up_t(v, S);
}
template <int XL, int S, typename T>
__device__ __forceinline__ T xl_sel_down(T v) {
    if constexpr ((XL & S) != 0) return xl_down<S>(v);
    else return shfl_down_t(v, S);
}

// value at level k-1 for every level a lane owns (fill at k = 0)
template <int E, int XL = 0>
__device__ __forceinline__ void shift_prev(const double (&a)[E], double (&o)[E], int lane, double fill) {
    double up;
    if constexpr ((XL & 1) != 0) up = xl_up<1>(a[E - 1]);
    else up = __shfl_up(a[E - 1], 1, 64);
    o[0] = (lane == 0) ? fill : up;
#pragma unroll
    for (int e = 1; e < E; ++e) o[e] = a[e - 1];
}
// value at level k+1 for every level a lane owns (fill past the last lane)
template <int E, int XL = 0>
__device__ __forceinline__ void shift_next(const double (&a)[E], double (&o)[E], int lane, double fill) {
    double dn;
    if constexpr ((XL & 1) != 0) dn = xl_down<1>(a[0]);
    else dn = __shfl_down(a[0], 1, 64);
    o[E - 1] = (lane == 63) ? fill : dn;
#pragma unroll
    for (int e = 0; e < E - 1; ++e) o[e] = a[e + 1];
}

// Memory policy MP of the column accessors.  0: plain loads and stores -- one kernel launch per phase, the
// launch boundary orders everything.  1: agent-coherent accesses (relaxed agent-scope atomics = `sc1` loads and
// stores on gfx950: the load bypasses the CU's L1, the store is written through) for data that OTHER workgroups
// of a persistent launch read or write between two grid barriers (the one-launch years and the command stream): an array accessed with
// MP = 1 anywhere in such a launch must be accessed with MP = 1 everywhere in it.
// MP = 1: data other workgroups anywhere on the chip exchange inside a launch -- write-through (sc1) stores, L1-bypassing
// (sc1) loads.  MP = 2: the same between workgroups that all sit on ONE XCD -- plain stores (they reach, and stay in, the
// XCD's L2 once the wave has waited for them) and the same L1-bypassing loads, which that L2 then serves.
template <int MP>
__device__ __forceinline__ double ld_mp(const double* p) {
    if constexpr (MP >= 1) {
        const unsigned long long bits = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
        return __longlong_as_double((long long)bits);
    } else {
        return *p;
    }
}
template <int MP>
__device__ __forceinline__ void st_mp(double* p, double v) {
    if constexpr (MP == 1) {
        __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    } else {
        *p = v;
    }
}

template <int E, int MP = 0>
__device__ __forceinline__ void load_col(const double* __restrict__ base, size_t col, int lane, double (&o)[E]) {
    const double* p = base + col * (size_t)(E * 64) + lane;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = ld_mp<MP>(p + e * 64);
}
template <int E, int MP = 0>
__device__ __forceinline__ void store_col(double* __restrict__ base, size_t col, int lane, const double (&v)[E]) {
    double* p = base + col * (size_t)(E * 64) + lane;
#pragma unroll
    for (int e = 0; e < E; ++e) st_mp<MP>(p + e * 64, v[e]);
}

// Tridiagonal solve of one column held by one wave (E consecutive rows per lane):
//     a[i] x[i-1] + d[i] x[i] + c[i] x[i+1] = r[i]
// a, c real; d, r real or complex.  Rows past the column end must be identity rows
// (a = c = 0, d = 1, r = 0).  Partition method: each lane eliminates inside its block
// of E rows (two sweeps), the 64 block-end unknowns form a tridiagonal system that is
// solved by parallel cyclic reduction with wave shuffles, then the interior unknowns
// follow by substitution.  No pivoting: the matrices here are strictly diagonally
// dominant (shifted M-matrices).
// ---------------------------------------------------------------------------------
// The solve is split in two.  The matrix-only part (pivot
// reciprocals, the coupling g to the next lane's first row, the parallel-cyclic-reduction
// multipliers of the 64 block-end unknowns and the final pivot) depends only on
// (shift, Jacobian planes), i.e. on SciPy's "LU" event, while a relaxation solve runs
// sweeps x Newton iterations x steps right-hand sides through it.  `tridiag_factor`
// computes that part once; `tridiag_apply` then needs no division and only two shuffles
// of the right-hand side per PCR level (instead of eight values).
// Table layout per lane: K1[6], K2[6], IB, G  (NK2D_TAB = 14 values of T).
// ---------------------------------------------------------------------------------
#define NK2D_TAB 14

// both directions of one value at distance S with the helper family XL (the lane's own value where it has no partner, either way)
template <int XL, int S, typename T>
__device__ __forceinline__ void xl_sel_both(T v, T& up, T& dn) {
    if constexpr ((XL & S) != 0) {
        if constexpr (sizeof(T) == sizeof(double)) {
            xl_both<S>(v, up, dn);
        } else {
            xl_both<S>(v.re, up.re, dn.re);
            xl_both<S>(v.im, up.im, dn.im);
        }
    } else {
        up = shfl_up_t(v, S);
        dn = shfl_down_t(v, S);
    }
}
// one level of tridiag_factor's parallel cyclic reduction with the helper family XL: the expressions of its loop, S a constant
template <int XL, int S, typename T>
__device__ __forceinline__ void pcr_factor_level(T& A, T& B, T& C, T& k1o, T& k2o, int lane) {
    T iB = t_recip(B);
    T Am, iBm, Cm, Ap, iBp, Cp;
    xl_sel_both<XL, S>(A, Am, Ap);
    xl_sel_both<XL, S>(iB, iBm, iBp);
    xl_sel_both<XL, S>(C, Cm, Cp);
    const bool hm = lane >= S, hp = lane + S < 64;
    T k1 = hm ? t_mul(A, iBm) : t_zero(T());
    T k2 = hp ? t_mul(C, iBp) : t_zero(T());
    if (!hm) { Am = t_zero(T()); Cm = t_zero(T()); }
    if (!hp) { Ap = t_zero(T()); Cp = t_zero(T()); }
    k1o = k1;
    k2o = k2;
    B = t_nfma(t_nfma(B, Cm, k1), Ap, k2);
    A = t_neg(t_mul(Am, k1));
    C = t_neg(t_mul(Cp, k2));
}

template <int E, typename T, int XL = 0>
__device__ __forceinline__ void tridiag_factor(const double (&a)[E], const double (&c)[E], const T (&d)[E],
                                               T (&inv)[E], T (&tab)[NK2D_TAB], int lane) {
    T al[E], be[E];
    T dlast = d[0];
    inv[0] = t_recip(d[0]);
    al[0] = t_from_real(a[0], T());
#pragma unroll
    for (int i = 1; i < E; ++i) {
        T m = t_mulr(inv[i - 1], a[i]);
        T dd = t_nfmar(d[i], m, c[i - 1]);
        dlast = dd;
        inv[i] = t_recip(dd);
        al[i] = t_neg(t_mul(m, al[i - 1]));
    }
    T A, B, C, G;
    if constexpr (E >= 2) {
        be[E - 1] = t_zero(T());
        be[E - 2] = t_from_real(c[E - 2], T());
#pragma unroll
        for (int i = E - 3; i >= 0; --i) {
            T m = t_mulr(inv[i + 1], c[i]);
            al[i] = t_nfma(al[i], m, al[i + 1]);
            be[i] = t_neg(t_mul(m, be[i + 1]));
        }
        T n_al = xl_sel_down<XL, 1>(al[0]), n_inv = xl_sel_down<XL, 1>(inv[0]), n_be = xl_sel_down<XL, 1>(be[0]);
        G = t_mulr(n_inv, c[E - 1]);
        A = al[E - 1];
        B = t_nfma(dlast, G, n_al);
        C = t_neg(t_mul(G, n_be));
    } else {
        G = t_zero(T());
        A = t_from_real(a[0], T());
        B = d[0];
        C = t_from_real(c[0], T());
    }
    if constexpr (XL != 0) {
        pcr_factor_level<XL, 1>(A, B, C, tab[0], tab[6], lane);
        pcr_factor_level<XL, 2>(A, B, C, tab[1], tab[7], lane);
        pcr_factor_level<XL, 4>(A, B, C, tab[2], tab[8], lane);
        pcr_factor_level<XL, 8>(A, B, C, tab[3], tab[9], lane);
        pcr_factor_level<XL, 16>(A, B, C, tab[4], tab[10], lane);
        pcr_factor_level<XL, 32>(A, B, C, tab[5], tab[11], lane);
    } else {
    int lv = 0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1, ++lv) {
        T iB = t_recip(B);
        T Am = shfl_up_t(A, s), iBm = shfl_up_t(iB, s), Cm = shfl_up_t(C, s);
        T Ap = shfl_down_t(A, s), iBp = shfl_down_t(iB, s), Cp = shfl_down_t(C, s);
        const bool hm = lane >= s, hp = lane + s < 64;
        T k1 = hm ? t_mul(A, iBm) : t_zero(T());
        T k2 = hp ? t_mul(C, iBp) : t_zero(T());
        if (!hm) { Am = t_zero(T()); Cm = t_zero(T()); }
        if (!hp) { Ap = t_zero(T()); Cp = t_zero(T()); }
        tab[lv] = k1;
        tab[6 + lv] = k2;
        B = t_nfma(t_nfma(B, Cm, k1), Ap, k2);
        A = t_neg(t_mul(Am, k1));
        C = t_neg(t_mul(Cp, k2));
    }
    }
    tab[12] = t_recip(B);
    tab[13] = G;
}

// one level of tridiag_apply's parallel cyclic reduction with the helper family XL
template <int XL, int S, typename T>
__device__ __forceinline__ T pcr_apply_level(T R, T k1, T k2) {
    T Rm, Rp;
    if constexpr ((XL & S) != 0) {
        if constexpr (sizeof(T) == sizeof(double)) {
            xl_both<S>(R, Rm, Rp);
        } else {
            xl_both<S>(R.re, Rm.re, Rp.re);
            xl_both<S>(R.im, Rm.im, Rp.im);
        }
    } else {
        Rm = shfl_up_t(R, S);
        Rp = shfl_down_t(R, S);
    }
    return t_nfma(t_nfma(R, Rm, k1), Rp, k2);
}

template <int E, typename T, int XL = 0>
__device__ __forceinline__ void tridiag_apply(const double (&a)[E], const double (&c)[E], const T (&inv)[E],
                                              const T (&tab)[NK2D_TAB], T (&r)[E], int lane) {
    T al[E], be[E];
    al[0] = t_from_real(a[0], T());
#pragma unroll
    for (int i = 1; i < E; ++i) {
        T m = t_mulr(inv[i - 1], a[i]);
        r[i] = t_nfma(r[i], m, r[i - 1]);
        al[i] = t_neg(t_mul(m, al[i - 1]));
    }
    T R;
    if constexpr (E >= 2) {
        be[E - 1] = t_zero(T());
        be[E - 2] = t_from_real(c[E - 2], T());
#pragma unroll
        for (int i = E - 3; i >= 0; --i) {
            T m = t_mulr(inv[i + 1], c[i]);
            r[i] = t_nfma(r[i], m, r[i + 1]);
            al[i] = t_nfma(al[i], m, al[i + 1]);
            be[i] = t_neg(t_mul(m, be[i + 1]));
        }
        T n_r = xl_sel_down<XL, 1>(r[0]);
        R = t_nfma(r[E - 1], tab[13], n_r);
    } else {
        R = r[0];
    }
    if constexpr (XL != 0) {
        R = pcr_apply_level<XL, 1>(R, tab[0], tab[6]);
        R = pcr_apply_level<XL, 2>(R, tab[1], tab[7]);
        R = pcr_apply_level<XL, 4>(R, tab[2], tab[8]);
        R = pcr_apply_level<XL, 8>(R, tab[3], tab[9]);
        R = pcr_apply_level<XL, 16>(R, tab[4], tab[10]);
        R = pcr_apply_level<XL, 32>(R, tab[5], tab[11]);
    } else {
    int lv = 0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1, ++lv) {
        T Rm = shfl_up_t(R, s), Rp = shfl_down_t(R, s);  // multipliers are 0 where no partner
        R = t_nfma(t_nfma(R, Rm, tab[lv]), Rp, tab[6 + lv]);
    }
    }
    T xl = t_mul(R, tab[12]);
    T xp = xl_sel_up<XL, 1>(xl);
    if (lane == 0) xp = t_zero(T());
    if constexpr (E >= 2) {
#pragma unroll
        for (int i = 0; i < E - 1; ++i) {
            T v = t_nfma(t_nfma(r[i], al[i], xp), be[i], xl);
            r[i] = t_mul(inv[i], v);
        }
    }
    r[E - 1] = xl;
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------------
// host-side entry points implemented across the translation units
// ---------------------------------------------------------------------------------
// nk2d_kernels.hip
int nk2d_k_pack_plane(nk2d_ctx* c, const double* src_dev, int nrows, int ncols, double* dst, double fill);
int nk2d_k_pack_state(nk2d_ctx* c, const double* src_dev, double* dst);
int nk2d_k_unpack_state(nk2d_ctx* c, const double* src, double* dst_dev);
int nk2d_k_unpack_plane(nk2d_ctx* c, const double* src, int nrows, int ncols, double* dst_dev);
int nk2d_k_vmix(nk2d_ctx* c, int nt, const double* times, double* const* out);
int nk2d_k_tend(nk2d_ctx* c, const double* y, const double* kv, double* f);
int nk2d_k_jac(nk2d_ctx* c, const double* kv, const double* ylin);
int nk2d_k_jac_apply(nk2d_ctx* c, const double* v, double* out);
int nk2d_k_sweep(nk2d_ctx* c, bool do_real, bool do_cplx, bool first, double cre, double ccr, double cci,
                 const double* br, const double* bcr, const double* bci, int src);
int nk2d_k_factor(nk2d_ctx* c, bool do_real, bool do_cplx, double cre, double ccr, double cci);
int nk2d_k_reduce(nk2d_ctx* c, int ntasks, int nout, double* host_out);
int nk2d_part_sum(nk2d_ctx* c, int ntasks, double* out, const double* part);
int nk2d_r_err_fused(nk2d_ctx* c, double h, int m, int* buf, double* part);
int nk2d_r_commit_tend(nk2d_ctx* c, const double* kv);
int nk2d_r_step_boundary(nk2d_ctx* c, const double* kv_new, bool do_jac, const double* times, double* const* out,
                         double x0, double x1, double x2, int jac_stage = -1, bool with_tend = true);
int nk2d_r_rows_sum(nk2d_ctx* c, const double* rows, int64_t nrows, double* out);
int nk2d_r_newton_final(nk2d_ctx* c, bool do_stage, bool first, double mreal, double mcr, double mci, int src, bool delta,
                        const double* times, double x0, double x1, double x2, int jac_stage);
int nk2d_r_attempt_setup(nk2d_ctx* c, const double* times, double* const* out, double x0, double x1, double x2,
                         int jac_stage = -1);
double nk2d_fingerprint(const nk2d_ctx* c);
uint64_t nk2d_frozen_key(const nk2d_ctx* c, const double* sched, int64_t n);   // schedule ^ fingerprint ^ frozen_err_check
int nk2d_frozen_persistent(nk2d_ctx* c, const double* sched, int64_t n, std::vector<char>* err_rows = nullptr);
int nk2d_frozen_cache_pending(const nk2d_ctx* c);
int64_t nk2d_frozen_cache_npieces(const nk2d_ctx* c);
int64_t nk2d_frozen_cache_piece_allocs(const nk2d_ctx* c);
// option "frozen_cache_early": the pieces of the schedule a free-running year just recorded, asked for from a thread
int nk2d_frozen_cache_early(nk2d_ctx* c, const double* sched, int64_t n);
int64_t nk2d_frozen_cache_bytes(const nk2d_ctx* c);
int nk2d_frozen_cache_is_lean(const nk2d_ctx* c);      // 1 while the cache the context holds is lean (option "frozen_cache_lean")
void nk2d_frozen_cache_free(nk2d_ctx* c);
int nk2d_prof_window_begin(nk2d_ctx* c);
int nk2d_prof_window_end(nk2d_ctx* c);
int nk2d_host_interp(int n, const double* xp, const double* fp, double x, double* out);
int nk2d_sweeps_for(nk2d_ctx* c, double c_real);
bool nk2d_has_lateral(const nk2d_ctx* c);
int nk2d_profile_collect(nk2d_ctx* c);
int nk2d_r_predict(nk2d_ctx* c, double x0, double x1, double x2);
int nk2d_r_newton_fused(nk2d_ctx* c, bool do_stage, bool first, bool do_update, double mreal, double mcr,
                        double mci, int src, bool delta);
int nk2d_r_err_rhs(nk2d_ctx* c, double h);
int nk2d_r_err_rhs2(nk2d_ctx* c, const double* err, double h);
int nk2d_r_err_norm(nk2d_ctx* c, const double* err);
int nk2d_r_copy(nk2d_ctx* c, double* dst, const double* src);
int nk2d_r_wnorm(nk2d_ctx* c, const double* a, const double* b, double ca, double cb, const double* ys);
int nk2d_r_axpy(nk2d_ctx* c, const double* a, double s, const double* b, double* out);
int nk2d_r_final(nk2d_ctx* c, const double* y0, double* out);
int nk2d_r_dense(nk2d_ctx* c, double x, double* out);
// nk2d_radau.hip
int nk2d_hist_sample(nk2d_ctx* c, double t_old, double t_new, bool first);
// the next sample of the running year if it is due in the accepted step (t_old, t_new), and its dense-output abscissa: ONE
// expression for the samples by launches (nk2d_hist_sample) and by commands (nk2d_hist_push) -- they must give the same bits
static inline bool nk2d_hist_due(const nk2d_ctx* c, double t_old, double t_new, double* x) {
    if (!(c->hist_next < c->hist_n && c->hist_t[c->hist_next] <= t_new)) return false;
    const double te = c->hist_t[c->hist_next];
    *x = (te - t_old) / (t_new - t_old);
    return true;
}
// option "stream_hist": the sample buffer in place before the year; the samples due at t_new as commands; the buffered
// samples to the host (launches: ends a running kernel); the bookkeeping of a year that is given up
int nk2d_hist_buf_ready(nk2d_ctx* c);
int nk2d_hist_push(nk2d_ctx* c, double t_old, double t_new);
int nk2d_hist_drain(nk2d_ctx* c);
void nk2d_hist_buf_reset(nk2d_ctx* c);
void nk2d_hist_year_done(nk2d_ctx* c);
int nk2d_r_dense_push(nk2d_ctx* c, double x, double* out);
int nk2d_radau_year(nk2d_ctx* c, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, const double* replay,
                    int64_t replay_n, double* record, int64_t record_cap, int64_t* record_n, bool replay_own = false);
// nk2d_precond.hip
void nk2d_precond_free(nk2d_ctx* c);
// the current factorisation is the extrapolated phosphorus preconditioner (nk2d_precond_setup_states with the null vector since the last factorisation)
bool nk2d_precond_has_nullspace(const nk2d_ctx* c);
