// nk2d_api.hip -- C ABI entry points (include/nk2d.h): context life cycle, layout
// conversion, region-weighted state algebra (dot / axpby / lin_comb / MGS) and thin
// wrappers over the model kernels.
#include "nk2d_common.h"
#include "nk2d_build_id.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace {

template <typename T>
int dev_alloc(nk2d_ctx* c, T** p, size_t n) {
    NK2D_CHECK(c, hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
    NK2D_CHECK(c, hipMemsetAsync(*p, 0, sizeof(T) * std::max<size_t>(n, 1), nk2d_s(c)));
    return 0;
}

// STAGE (device) holds a host-layout copy for the pack / unpack kernels; hSTAGE is its pinned host
// twin.  Host arrays of the caller are pageable: copying them straight to / from the device makes
// the runtime pin the pages on the fly (milliseconds per call), so they go through hSTAGE.
int ensure_stage(nk2d_ctx* c, size_t n) {
    if (n <= c->stage_elems) return 0;
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    if (c->STAGE) NK2D_CHECK(c, hipFree(c->STAGE));
    if (c->hSTAGE) NK2D_CHECK(c, hipHostFree(c->hSTAGE));
    c->STAGE = c->hSTAGE = nullptr;
    c->stage_elems = 0;
    NK2D_CHECK(c, hipMalloc((void**)&c->STAGE, sizeof(double) * n));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hSTAGE, sizeof(double) * n));
    c->stage_elems = n;
    return 0;
}

// host (pageable) -> STAGE
int stage_in(nk2d_ctx* c, const double* host, size_t n) {
    NK2D_TRY(ensure_stage(c, n));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));  // hSTAGE may still feed an earlier copy
    std::memcpy(c->hSTAGE, host, sizeof(double) * n);
    NK2D_CHECK(c, hipMemcpyAsync(c->STAGE, c->hSTAGE, sizeof(double) * n, hipMemcpyHostToDevice, nk2d_s(c)));
    return 0;
}

// STAGE -> host (pageable); returns with the copy complete
int stage_out(nk2d_ctx* c, double* host, size_t n) {
    NK2D_CHECK(c, hipMemcpyAsync(c->hSTAGE, c->STAGE, sizeof(double) * n, hipMemcpyDeviceToHost, nk2d_s(c)));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    std::memcpy(host, c->hSTAGE, sizeof(double) * n);
    return 0;
}

}  // namespace

// staging pairs of the two-half downloads (nk2d_vec_download_begin / _end)
struct nk2d_download {
    double* dev = nullptr;     // host-layout copy on the device
    double* host = nullptr;    // pinned
    hipEvent_t done = nullptr; // behind the copy into `host`
    size_t n = 0;
};
struct nk2d_download_pool {
    std::mutex m;
    std::vector<nk2d_download*> all, idle;
};

namespace {

void download_pool_free(nk2d_ctx* c) {
    if (!c->dl_pool) return;
    for (nk2d_download* t : c->dl_pool->all) {
        (void)hipEventSynchronize(t->done);
        (void)hipEventDestroy(t->done);
        (void)hipFree(t->dev);
        (void)hipHostFree(t->host);
        delete t;
    }
    delete c->dl_pool;
    c->dl_pool = nullptr;
}

// host row-major [nrows][ncols] -> packed device plane of ncols columns
int upload_plane(nk2d_ctx* c, const double* host, int nrows, int ncols, double* dst, double fill = 0.0) {
    const size_t n = (size_t)nrows * ncols;
    NK2D_TRY(stage_in(c, host, n));
    NK2D_TRY(nk2d_k_pack_plane(c, c->STAGE, nrows, ncols, dst, fill));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}

void build_front(nk2d_ctx* c, const std::vector<double>& dzr, const std::vector<double>& dyr) {
    const int nz = c->nz, ny = c->ny;
    const double* v = c->d.vvel;
    const double* w = c->d.wvel;
    const double* kh = c->d.hmix_coeff;
    std::vector<std::pair<double, double>> pts;  // (q, s)
    pts.reserve((size_t)nz * ny);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j) {
            const double a_up = (k > 0) ? (-0.5 * w[(size_t)k * ny + j]) * dzr[k] : 0.0;
            const double a_dn = (k < nz - 1) ? (0.5 * w[(size_t)(k + 1) * ny + j]) * dzr[k] : 0.0;
            const double a_s = (j > 0) ? (0.5 * v[(size_t)k * (ny + 1) + j]) * dyr[j] : 0.0;
            const double a_n = (j < ny - 1) ? (-0.5 * v[(size_t)k * (ny + 1) + j + 1]) * dyr[j] : 0.0;
            const double h_s = (j > 0) ? kh[(size_t)k * (ny - 1) + j - 1] * dyr[j] : 0.0;
            const double h_n = (j < ny - 1) ? kh[(size_t)k * (ny - 1) + j] * dyr[j] : 0.0;
            const double s = std::fabs(a_s + h_s) + std::fabs(a_n + h_n);
            const double q = (h_s + h_n) - (a_s + a_n) - 2.0 * (a_up + a_dn);
            if (c->kind == 1) {
                // rows of po4 / dop / pop: the coupling to the other tracers of the cell is relaxed with
                // the lateral terms (s), the module's diagonal and sinking terms change the margin (q);
                // d uptake / d po4 <= max_rate * light / halfsat for po4 >= 0
                const double* ph = c->d.phos_params;
                const double upr_max = ph[1] * c->d.light_lim[(size_t)k * ny + j] / ph[0];
                const double sink_out = (k < nz - 1) ? ph[5] * dzr[k] : 0.0, sink_in = (k > 0) ? ph[5] * dzr[k] : 0.0;
                pts.emplace_back(q, s + ph[3] + ph[4]);
                pts.emplace_back(q + ph[3], s + ph[2] * upr_max);
                pts.emplace_back(q + ph[4] + sink_out - sink_in, s + (1.0 - ph[2]) * upr_max);
            } else if (s > 0.0) {
                pts.emplace_back(q, s);
            }
        }
    // tabulate rho(c) for c = c0 * 10^(k * dlog)
    c->rho_c0 = 1.0e-10;
    c->rho_dlog = 1.0 / 64.0;
    const int ntab = 64 * 15;
    c->rho_tab.assign(ntab, 0.0);
    for (int k = 0; k < ntab; ++k) {
        const double shift = c->rho_c0 * std::pow(10.0, k * c->rho_dlog);
        double rho = 0.0;
        for (const auto& p : pts) {
            const double den = shift + p.first;
            const double r = (den > 0.0) ? p.second / den : 1.0e30;
            if (r > rho) rho = r;
        }
        c->rho_tab[k] = rho;
    }
}

}  // namespace

extern "C" const char* nk2d_version(void) { return "nk2d 0.1 (gfx950)"; }

extern "C" const char* nk2d_last_error(const nk2d_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" void* nk2d_stream(nk2d_ctx* ctx) { return ctx ? (void*)nk2d_s(ctx) : nullptr; }

// Self-test of the VALU cross-lane moves (the xl_ helpers of nk2d_common.h), reached through options and counters -- the C ABI
// keeps its entry points.  Options "xlane_selftest_in0" .. "xlane_selftest_in63" take the 64 doubles of one wave, lane by lane (a
// double passes a NaN's payload on untouched); option "xlane_selftest_run" 1 lets one wave apply every helper at every distance
// to them (a complex value: the vector as the real part, the vector read backwards as the imaginary part); counter
// "xlane_selftest_<w>_<row>_<lane>" is then the 64 bits lane <lane> holds of row <row>, by __shfl (w = 0) and by the helper (w = 1).
// Rows: 0-5 up and 6-11 down by 1, 2, 4, 8, 16, 32 lanes; 12-17 / 18-23 the complex up (re / im), 24-29 / 30-35 the complex down;
// 36 the sum over the wave (only lane 0 holds the total).
#define NK2D_XLANE_SELFTEST_ROWS 37
static double xl_selftest_in[64];
static int64_t xl_selftest_out[2 * NK2D_XLANE_SELFTEST_ROWS * 64];
template <int S>
__device__ __forceinline__ void xlane_selftest_rows(double v, cplx z, int lv, int lane, double* __restrict__ ref, double* __restrict__ got) {
    ref[(0 + lv) * 64 + lane] = __shfl_up(v, S, 64);            got[(0 + lv) * 64 + lane] = xl_up<S>(v);
    ref[(6 + lv) * 64 + lane] = __shfl_down(v, S, 64);          got[(6 + lv) * 64 + lane] = xl_down<S>(v);
    const cplx ru = shfl_up_t(z, S), gu = xl_up<S>(z), rd = shfl_down_t(z, S), gd = xl_down<S>(z);
    ref[(12 + lv) * 64 + lane] = ru.re;                         got[(12 + lv) * 64 + lane] = gu.re;
    ref[(18 + lv) * 64 + lane] = ru.im;                         got[(18 + lv) * 64 + lane] = gu.im;
    ref[(24 + lv) * 64 + lane] = rd.re;                         got[(24 + lv) * 64 + lane] = gd.re;
    ref[(30 + lv) * 64 + lane] = rd.im;                         got[(30 + lv) * 64 + lane] = gd.im;
}
__global__ __launch_bounds__(64) void k_xlane_selftest(const double* __restrict__ in, double* __restrict__ ref, double* __restrict__ got) {
    const int lane = (int)threadIdx.x;
    const double v = in[lane];
    const cplx z = c_make(v, in[63 - lane]);
    xlane_selftest_rows<1>(v, z, 0, lane, ref, got);
    xlane_selftest_rows<2>(v, z, 1, lane, ref, got);
    xlane_selftest_rows<4>(v, z, 2, lane, ref, got);
    xlane_selftest_rows<8>(v, z, 3, lane, ref, got);
    xlane_selftest_rows<16>(v, z, 4, lane, ref, got);
    xlane_selftest_rows<32>(v, z, 5, lane, ref, got);
    ref[36 * 64 + lane] = wave_sum(v);
    got[36 * 64 + lane] = xl_wave_sum(v);
}


static int xlane_selftest_run(nk2d_ctx* c) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    const size_t rows = NK2D_XLANE_SELFTEST_ROWS, n = 64 + 2 * rows * 64;
    NK2D_TRY(ensure_stage(c, n));
    NK2D_TRY(stage_in(c, xl_selftest_in, 64));
    k_xlane_selftest<<<1, 64, 0, nk2d_s(c)>>>(c->STAGE, c->STAGE + 64, c->STAGE + 64 + rows * 64);
    NK2D_CHECK(c, hipGetLastError());
    NK2D_CHECK(c, hipMemcpyAsync(c->hSTAGE, c->STAGE, sizeof(double) * n, hipMemcpyDeviceToHost, nk2d_s(c)));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    std::memcpy(xl_selftest_out, c->hSTAGE + 64, sizeof(double) * 2 * rows * 64);
    return 0;
}

extern "C" int nk2d_set_option(nk2d_ctx* c, const char* name, double value) {
    const std::string key(name ? name : "");
    if (key.rfind("xlane_selftest_in", 0) == 0) {
        const int lane = std::atoi(key.c_str() + 17);
        if (key.size() < 18 || lane < 0 || lane > 63) return nk2d_fail(c, "nk2d_set_option: xlane_selftest_in<lane> takes lanes 0 .. 63");
        xl_selftest_in[lane] = value;
        return 0;
    }
    if (key == "xlane_selftest_run") return (int)value != 0 ? xlane_selftest_run(c) : 0;
    if (key == "device_ctl") {
        // (rounds 1-3 had Newton decisions on the device -- 1, 2 -- and a one-launch year with the whole controller on the
        // device -- 3; all three lost to the host's controller driving ONE resident kernel, nk2d_stream.h, and are gone)
        if ((int)value != 0) return nk2d_fail(c, "nk2d_set_option: device_ctl 1, 2 and 3 no longer exist (the controller is the host's; see option stream_years)");
        return 0;
    }
    if (key == "jac_fresh") { c->jac_fresh = value != 0.0; return 0; }
    if (key == "growth_cap") {
        if (!(value >= 0.0)) return nk2d_fail(c, "nk2d_set_option: growth_cap must be >= 0");
        c->growth_cap = value;
        return 0;
    }
    if (key == "speculate") { c->speculate = value != 0.0; return 0; }
    if (key == "hook_spec_depth") {
        if (!(value == 1.0 || value == 2.0)) return nk2d_fail(c, "nk2d_set_option: hook_spec_depth is 1 or 2");
        c->hook_spec_depth = (int)value;
        return 0;
    }
    if (key == "pc_valu") { c->pc_valu = value != 0.0; return 0; }
    if (key == "pc_fused") { c->pc_fused = (int)value; return 0; }
    if (key == "pc_fp32") { c->pc_fp32 = value != 0.0; return 0; }
    if (key == "pc_refine") {
        if (!(value >= 0.0 && value <= 4.0)) return nk2d_fail(c, "nk2d_set_option: pc_refine must be 0 .. 4");
        c->pc_refine = (int)value;
        return 0;
    }
    if (key == "pc_two_ended") {
        // block elimination of the preconditioner from both ends of the ypos axis (nk2d_precond.hip); taken at the next set-up
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: pc_two_ended is 0 or 1");
        c->pc_two_ended = (int)value;
        return 0;
    }
    if (key == "pc_pivot_wave") {
        // pivot blocks of the preconditioner's Gauss-Jordan inversions by one wave in registers (nk2d_precond.hip); taken at
        // the next set-up
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: pc_pivot_wave is 0 or 1");
        c->pc_pivot_wave = (int)value;
        return 0;
    }
    if (key == "pc_panel") {
        // pivots per panel step of the preconditioner's Gauss-Jordan inversions (nk2d_precond.hip); taken at the next set-up
        if (value != 32.0 && value != 64.0) return nk2d_fail(c, "nk2d_set_option: pc_panel is 32 or 64");
        c->pc_panel = (int)value;
        return 0;
    }
    if (key == "final_fuse") { c->final_fuse = value != 0.0; return 0; }
    if (key == "year_fences") { c->year_fences = value != 0.0; return 0; }
    if (key == "frozen_persistent") { c->frozen_persistent = value != 0.0; return 0; }
    if (key == "frozen_team") { c->frozen_team = value != 0.0; return 0; }
    if (key == "frozen_coef_lds") { c->frozen_coef_lds = (int)value & 63; return 0; }
    if (key == "frozen_sums_poison") { c->frozen_sums_poison = (int)value != 0 ? 1 : 0; return 0; }
    if (key == "frozen_early") { c->frozen_early = (int)value != 0 ? 1 : 0; return 0; }
    if (key == "frozen_stage_exchange") { c->frozen_stage_exchange = (int)value != 0 ? 1 : 0; return 0; }
    if (key == "frozen_xlane") { c->frozen_xlane = (int)value != 0 ? 1 : 0; return 0; }
    if (key == "frozen_dedicated") {
        // the one-launch year in the entry that carries the default year's body alone (nk2d_frozen_d.hip); read at every frozen year
        if (value != 0.0 && value != 1.0 && value != 2.0) return nk2d_fail(c, "nk2d_set_option: frozen_dedicated is 0, 1 or 2");
        c->frozen_dedicated = (int)value;
        return 0;
    }
    if (key == "frozen_by_column") { c->frozen_by_column = (int)value; return 0; }
    if (key == "frozen_cache_after") { c->frozen_cache_after = (int)value; return 0; }
    if (key == "spec_bias") { c->spec_bias = value > 0.0 ? value : 1.0; return 0; }
    if (key == "stream_years") { c->stream_years = (int)value; c->stream_lost = 0; return 0; }
    if (key == "frozen_tape") {
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: frozen_tape is 0 or 1");
        c->frozen_tape = (int)value;
        return 0;
    }
    if (key == "stream_hist") {
        // history samples as commands of the year's resident kernel (nk2d_stream.h, NK2D_OP_DENSE_OUT) instead of launches
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: stream_hist is 0 or 1");
        c->stream_hist = (int)value;
        return 0;
    }
    if (key == "stream_hist_mb") {
        if (!(value >= 0.0) || !std::isfinite(value)) return nk2d_fail(c, "nk2d_set_option: stream_hist_mb must be >= 0");
        c->stream_hist_mb = value;
        return 0;
    }
    if (key == "stream_xlane") {
        // (no decision, no change of the resident kernel's shape: read at every start of the kernel, nk2d_stream.hip)
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: stream_xlane is 0 or 1");
        c->stream_xlane = (int)value;
        return 0;
    }
    if (key == "stream_two_waves") {
        // (decides the shape of the resident kernel: taken before the context's first year as a command stream)
        if (c->strm) return nk2d_fail(c, "nk2d_set_option: stream_two_waves must be set before the first year of the context");
        c->stream_two_waves = (int)value;
        return 0;
    }
    if (key == "frozen_wpb") { c->frozen_wpb = (int)value; return 0; }
    if (key == "frozen_alloc_async") { c->frozen_alloc_async = value != 0.0; return 0; }
    if (key == "frozen_persistent_max_e") { c->frozen_persistent_max_e = (int)value; return 0; }
    if (key == "frozen_cache_gb") { c->frozen_cache_max_gb = value; return 0; }
    if (key == "frozen_cache_pieces") {
        // the schedule cache as a list of equally sized pieces instead of one slab (nk2d_frozen.hip); taken at the next frozen year
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: frozen_cache_pieces is 0 or 1");
        c->frozen_cache_pieces = (int)value;
        return 0;
    }
    if (key == "frozen_cache_lean") {
        // the schedule cache without the factor tables (nk2d_frozen.hip): the one-launch year factorises in the first phase of every
        // step; 2: only where the full cache would be refused.  Taken when a cache is (re)built
        if (value != 0.0 && value != 1.0 && value != 2.0) return nk2d_fail(c, "nk2d_set_option: frozen_cache_lean is 0, 1 or 2");
        c->frozen_cache_lean = (int)value;
        return 0;
    }
    if (key == "frozen_forced") {
        // the one-launch year for the file-driven forced module where it has none by default (nk2d_frozen.hip).  Bit 1: linear sources at
        // five to eight levels per lane; bit 2: a thresholded sink, on the lean cache.  Taken at the next frozen year
        if (value != 0.0 && value != 1.0 && value != 2.0 && value != 3.0) return nk2d_fail(c, "nk2d_set_option: frozen_forced is a bit mask 0 ... 3");
        c->frozen_forced = (int)value;
        return 0;
    }
    if (key == "frozen_phosphorus") {
        // the one-launch year for the phosphorus module, on the lean cache at three to eight levels per lane (nk2d_frozen.hip).  1: one wave
        // per SIMD where its grid is resident; 2: else the 256-register flavour; 3: that flavour wherever it exists.  Taken at the next frozen year
        if (value != 0.0 && value != 1.0 && value != 2.0 && value != 3.0) return nk2d_fail(c, "nk2d_set_option: frozen_phosphorus is 0, 1, 2 or 3");
        c->frozen_phosphorus = (int)value;
        return 0;
    }
    if (key == "frozen_phosphorus_shallow") {
        // ... at one and two levels per lane too (nk2d_frozen.hip: the same by-column workgroup, nothing of the year in LDS).  Taken at
        // the next frozen year
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: frozen_phosphorus_shallow is 0 or 1");
        c->frozen_phosphorus_shallow = (int)value;
        return 0;
    }
    if (key == "frozen_cache_piece_mb") {
        if (!(value > 0.0) || !std::isfinite(value)) return nk2d_fail(c, "nk2d_set_option: frozen_cache_piece_mb must be > 0");
        c->frozen_cache_piece_mb = value;
        return 0;
    }
    if (key == "frozen_cache_piece_rows") {
        if (!(value >= 0.0) || value > 1.0e9) return nk2d_fail(c, "nk2d_set_option: frozen_cache_piece_rows must be 0 (from frozen_cache_piece_mb) or a row count");
        c->frozen_cache_piece_rows = (int64_t)value;
        return 0;
    }
    if (key == "frozen_cache_early") {
        if (value != 0.0 && value != 1.0) return nk2d_fail(c, "nk2d_set_option: frozen_cache_early is 0 or 1");
        c->frozen_cache_early = (int)value;
        return 0;
    }
    if (key == "barrier_timeout_ms") {
        if (!(value >= 0.0)) return nk2d_fail(c, "nk2d_set_option: barrier_timeout_ms must be >= 0");
        c->barrier_timeout_ms = value;
        return 0;
    }
    if (key == "frozen_err_check") {
        if (!(value >= 0.0) || value > 1.0e6) return nk2d_fail(c, "nk2d_set_option: frozen_err_check must be 0 (off) or a step stride");
        c->frozen_err_check = (int)value;
        return 0;
    }
    if (key == "jac_stage_state") { c->jac_stage_state = value != 0.0; return 0; }
    if (key == "jac_stage") {
        if (value != -1.0 && value != 0.0 && value != 1.0 && value != 2.0) return nk2d_fail(c, "nk2d_set_option: jac_stage must be -1, 0, 1 or 2");
        c->jac_stage = (int)value;
        return 0;
    }
    if (key == "team") {   // -1: automatic (see nk2d_team_auto), 0 / 1: never / always
        if (value != 0.0 && value != 1.0 && value != 2.0 && value != -1.0) return nk2d_fail(c, "nk2d_set_option: team must be -1, 0, 1 or 2");
        c->team = (value < 0.0) ? nk2d_team_auto(c) : (int)value;
        return 0;
    }
    if (key == "min_sweeps") {
        if (value != 1.0 && value != 2.0) return nk2d_fail(c, "nk2d_set_option: min_sweeps must be 1 or 2");
        c->min_sweeps = (int)value;
        c->yr_lin_tol = -1.0;   // the persistent kernel's sweep table is rebuilt
        return 0;
    }
    if (key == "factor_fp32") {
        // the single precision copy is written by the next factorisation: drop the cached one
        c->factor_fp32 = value != 0.0;
        return 0;
    }
    if (key == "sweep_wpb") {
        const int w = (int)value;
        if (w != 1 && w != 2 && w != 4) return nk2d_fail(c, "nk2d_set_option: sweep_wpb must be 1, 2 or 4");
        c->sweep_wpb = w;
        return 0;
    }
    if (key == "lin_tol") {
        if (!(value > 0.0 && value < 1.0)) return nk2d_fail(c, "nk2d_set_option: lin_tol must be in (0, 1)");
        c->d.lin_tol = value;
        return 0;
    }
    return nk2d_fail(c, "nk2d_set_option: unknown option " + key);
}

extern "C" int nk2d_sync(nk2d_ctx* c) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}

// ---------------------------------------------------------------------------------
// sampled timing of the dominant kernel (line-relaxation sweep) with HIP events on the
// context's own stream
// ---------------------------------------------------------------------------------
extern "C" int nk2d_profile_reset(nk2d_ctx* c, int32_t every_n) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    const size_t want = every_n > 0 ? 2 * 8192 : 0;
    while (c->prof_ev.size() < want) {
        hipEvent_t e;
        NK2D_CHECK(c, hipEventCreate(&e));
        c->prof_ev.push_back(e);
    }
    // calibrate: what an event pair reads with nothing between the two records
    c->prof_overhead_ms = 0.0;
    if (every_n > 0) {
        const int ncal = 64;
        for (int i = 0; i < ncal; ++i) {
            NK2D_CHECK(c, hipEventRecord(c->prof_ev[2 * i], nk2d_s(c)));
            NK2D_CHECK(c, hipEventRecord(c->prof_ev[2 * i + 1], nk2d_s(c)));
        }
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        double sum = 0.0;
        for (int i = 0; i < ncal; ++i) {
            float ms = 0.f;
            NK2D_CHECK(c, hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
            sum += ms;
        }
        c->prof_overhead_ms = sum / ncal;
    }
    c->prof_every = every_n;
    c->prof_used = 0;
    c->prof_ms_sum = 0.0;
    c->prof_cnt = 0;
    c->prof_windows = 0;
    c->prof_win_launches.clear();
    c->win_open = 0;
    c->win_seq = 0;
    c->sweep_launches = 0;
    c->sweep_bytes = 0.0;
    c->fused_bytes_all = 0.0;
    for (int i = 0; i < 4; ++i) { c->shape_cnt[i] = 0; c->shape_bytes[i] = 0.0; }
    return 0;
}

extern "C" int nk2d_profile_totals(nk2d_ctx* c, int64_t* launches, double* bytes) {
    if (launches) *launches = c->sweep_launches;
    if (bytes) *bytes = c->fused_bytes_all;
    return 0;
}

extern "C" int nk2d_profile_shapes(nk2d_ctx* c, int64_t* counts4, double* bytes4) {
    for (int i = 0; i < 4; ++i) {
        if (counts4) counts4[i] = c->shape_cnt[i];
        if (bytes4) bytes4[i] = c->shape_bytes[i];
    }
    return 0;
}

extern "C" int nk2d_timer_begin(nk2d_ctx* c) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (!c->timer_ready) {
        NK2D_CHECK(c, hipEventCreate(&c->timer_ev[0]));
        NK2D_CHECK(c, hipEventCreate(&c->timer_ev[1]));
        c->timer_ready = 1;
    }
    NK2D_CHECK(c, hipEventRecord(c->timer_ev[0], nk2d_s(c)));
    return 0;
}

extern "C" int nk2d_timer_end(nk2d_ctx* c, double* elapsed_ms) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (!c->timer_ready) return nk2d_fail(c, "nk2d_timer_end: nk2d_timer_begin was not called");
    NK2D_CHECK(c, hipEventRecord(c->timer_ev[1], nk2d_s(c)));
    NK2D_CHECK(c, hipEventSynchronize(c->timer_ev[1]));
    float ms = 0.f;
    NK2D_CHECK(c, hipEventElapsedTime(&ms, c->timer_ev[0], c->timer_ev[1]));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
}

extern "C" int nk2d_set_norm_hook(nk2d_ctx* c, nk2d_norm_hook_fn fn, void* user, double global_n) {
    if (fn && !(global_n >= (double)c->tc * c->nz * c->ny))
        return nk2d_fail(c, "nk2d_set_norm_hook: global_n must be at least this context's tc * nz * ny");
    c->norm_hook = fn;
    c->norm_hook_vec = nullptr;
    c->norm_hook_user = fn ? user : nullptr;
    c->global_n = fn ? global_n : 0.0;
    return 0;
}

// the scalar hook of a context that has a vector hook: one sum through the vector call
static double norm_hook_through_vec(void* user, double local_sum) {
    nk2d_ctx* c = (nk2d_ctx*)user;
    double v = local_sum;
    c->norm_hook_vec(c->norm_hook_vec_user, &v, 1);
    return v;
}

extern "C" int nk2d_set_norm_hook_vec(nk2d_ctx* c, nk2d_norm_hook_vec_fn fn, void* user, double global_n) {
    if (fn && !(global_n >= (double)c->tc * c->nz * c->ny))
        return nk2d_fail(c, "nk2d_set_norm_hook_vec: global_n must be at least this context's tc * nz * ny");
    if (fn && !c->ZS) {
        NK2D_CHECK(c, hipSetDevice(c->dev));
        NK2D_TRY(dev_alloc(c, &c->ZS, 3 * c->nv));
    }
    c->norm_hook_vec = fn;
    c->norm_hook_vec_user = fn ? user : nullptr;
    c->norm_hook = fn ? norm_hook_through_vec : nullptr;
    c->norm_hook_user = fn ? (void*)c : nullptr;
    c->global_n = fn ? global_n : 0.0;
    return 0;
}

extern "C" int nk2d_profile_read(nk2d_ctx* c, double* avg_us, int64_t* samples, int64_t* launches, double* bytes,
                                 double* overhead_us, int64_t* windows) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    NK2D_TRY(nk2d_profile_collect(c));
    // per launch: (sum of window times - one empty-pair reading per window) / launches in the windows
    const double net_ms = c->prof_ms_sum - (double)c->prof_windows * c->prof_overhead_ms;
    if (avg_us) *avg_us = c->prof_cnt > 0 ? 1000.0 * net_ms / (double)c->prof_cnt : 0.0;
    if (overhead_us) *overhead_us = 1000.0 * c->prof_overhead_ms;
    if (samples) *samples = c->prof_cnt;
    if (launches) *launches = c->sweep_launches;
    if (bytes) *bytes = c->sweep_bytes;
    if (windows) *windows = c->prof_windows;
    return 0;
}

// FNV-1a over raw bytes
static uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
template <class T>
static uint64_t fnv_val(uint64_t h, const T& v) { return fnv1a(h, &v, sizeof(T)); }

// everything a recorded schedule depends on besides the state (nk2d_schedule_fingerprint): the grid and module
// description hashed at create, the tolerances, the controller options that change the discrete map, and the BUILD of the
// library (NK2D_BUILD_ID: a checksum of its sources, csrc/Makefile -- a schedule from a side file another build wrote is
// refused, not replayed by kernels that may compute something else).  Options that select between bit-identical flavours of
// the same launches ("team", "final_fuse", "frozen_persistent", ...: each tested bit for bit against the others) are not part.
double nk2d_fingerprint(const nk2d_ctx* c) {
    uint64_t h = c->grid_hash;
    const char* ver = nk2d_version();
    h = fnv1a(h, ver, std::strlen(ver));
    h = fnv1a(h, NK2D_BUILD_ID, std::strlen(NK2D_BUILD_ID));
    h = fnv_val(h, c->d.rtol); h = fnv_val(h, c->d.atol); h = fnv_val(h, c->d.max_step_frac);
    h = fnv_val(h, c->d.t0); h = fnv_val(h, c->d.t1); h = fnv_val(h, c->d.lin_tol);
    h = fnv_val(h, c->jac_fresh); h = fnv_val(h, c->jac_stage); h = fnv_val(h, c->jac_stage_state);
    h = fnv_val(h, c->min_sweeps); h = fnv_val(h, c->growth_cap); h = fnv_val(h, c->factor_fp32);
    h &= (1ull << 52) - 1;
    return (double)(h ? h : 1ull);
}

static int create_impl(nk2d_ctx* c, const nk2d_desc* desc) {
    c->d = *desc;
    c->nz = desc->nz; c->ny = desc->ny; c->tc = desc->tc;
    c->kind = desc->module_kind;
    if (c->kind != 0 && c->kind != 1 && c->kind != 2) return nk2d_fail(c, "nk2d_create: unknown module_kind");
    c->SMSREC = c->RESTREC = nullptr;
    c->sms_t = c->rest_t = nullptr;
    if (c->kind == 2) {
        if (c->tc != 1) return nk2d_fail(c, "nk2d_create: the forced module has 1 tracer");
        if (desc->restore_nrec < 0 || desc->sms_nrec < 0 || desc->restore_nrec == 1 || desc->sms_nrec == 1)
            return nk2d_fail(c, "nk2d_create: a forcing set needs at least 2 records");
        if (desc->restore_nrec == 0 && desc->sms_nrec == 0)
            return nk2d_fail(c, "nk2d_create: module_kind 2 without forcing records (use module_kind 0)");
        if ((desc->restore_nrec > 0 && (!desc->restore_times || !desc->restore_vals)) ||
            (desc->sms_nrec > 0 && (!desc->sms_times || !desc->sms_vals)))
            return nk2d_fail(c, "nk2d_create: forcing records missing");
        if (desc->sink_thres < 0.0) return nk2d_fail(c, "nk2d_create: sink_thres < 0");
        for (int i = 1; i < desc->restore_nrec; ++i)
            if (!(desc->restore_times[i] > desc->restore_times[i - 1])) return nk2d_fail(c, "nk2d_create: restore_times not increasing");
        for (int i = 1; i < desc->sms_nrec; ++i)
            if (!(desc->sms_times[i] > desc->sms_times[i - 1])) return nk2d_fail(c, "nk2d_create: sms_times not increasing");
    } else {
        c->d.restore_nrec = c->d.sms_nrec = 0;
        c->d.sink_thres = 0.0;
    }
    if (c->kind == 1 && (c->tc != 3 || desc->light_lim == nullptr))
        return nk2d_fail(c, "nk2d_create: the phosphorus module has 3 tracers and needs light_lim");
    if (c->nz < 2 || c->ny < 1 || c->tc < 1 || c->tc > NK2D_MAX_TRACERS) return nk2d_fail(c, "nk2d_create: bad grid / tracer count");
    c->E = (c->nz + 63) / 64;
    if (c->E > NK2D_MAX_E) return nk2d_fail(c, "nk2d_create: nz > 512 levels not supported by this build");
    c->nzp = c->E * 64;
    c->ncol = c->tc * c->ny;
    c->nv = (size_t)c->ncol * c->nzp;
    c->np = (size_t)c->ny * c->nzp;
    c->kv_len = (c->kind == 2) ? 2 * c->np + (size_t)c->ny : c->np;
    c->nreg = 0;
    c->dev = desc->device_id;
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipStreamCreateWithFlags(&c->stream_, hipStreamNonBlocking));
    const int nz = c->nz, ny = c->ny;
    {
        uint64_t h = 14695981039346656037ull;
        h = fnv_val(h, c->nz); h = fnv_val(h, c->ny); h = fnv_val(h, c->tc); h = fnv_val(h, c->kind);
        h = fnv1a(h, desc->depth_edges, sizeof(double) * (nz + 1));
        h = fnv1a(h, desc->ypos_edges, sizeof(double) * (ny + 1));
        h = fnv1a(h, desc->vvel, sizeof(double) * (size_t)nz * (ny + 1));
        h = fnv1a(h, desc->wvel, sizeof(double) * (size_t)(nz + 1) * ny);
        if (ny > 1) h = fnv1a(h, desc->hmix_coeff, sizeof(double) * (size_t)nz * (ny - 1));
        h = fnv1a(h, desc->bldepth_max, sizeof(double) * ny);
        h = fnv_val(h, desc->bldepth_min); h = fnv1a(h, desc->bld_tvals, sizeof(desc->bld_tvals));
        h = fnv1a(h, desc->bld_fvals, sizeof(desc->bld_fvals));
        h = fnv_val(h, desc->vmix_log_shallow); h = fnv_val(h, desc->vmix_log_deep); h = fnv_val(h, desc->vmix_half_width);
        h = fnv1a(h, desc->surf_rate, sizeof(desc->surf_rate)); h = fnv1a(h, desc->surf_target, sizeof(desc->surf_target));
        h = fnv1a(h, desc->decay_rate, sizeof(desc->decay_rate)); h = fnv_val(h, desc->const_src);
        if (c->kind == 1) {
            h = fnv1a(h, desc->phos_params, sizeof(desc->phos_params));
            h = fnv1a(h, desc->light_lim, sizeof(double) * (size_t)nz * ny);
        }
        if (c->kind == 2) {
            h = fnv_val(h, c->d.restore_nrec); h = fnv_val(h, c->d.sms_nrec); h = fnv_val(h, c->d.sink_thres);
            if (c->d.restore_nrec > 0) {
                h = fnv1a(h, desc->restore_times, sizeof(double) * c->d.restore_nrec);
                h = fnv1a(h, desc->restore_vals, sizeof(double) * (size_t)c->d.restore_nrec * ny);
            }
            if (c->d.sms_nrec > 0) {
                h = fnv1a(h, desc->sms_times, sizeof(double) * c->d.sms_nrec);
                h = fnv1a(h, desc->sms_vals, sizeof(double) * (size_t)c->d.sms_nrec * nz * ny);
            }
        }
        c->grid_hash = h;
    }
    // ---- packed static planes
    NK2D_TRY(dev_alloc(c, &c->VV, (size_t)(ny + 1) * c->nzp));
    NK2D_TRY(dev_alloc(c, &c->KH, (size_t)(ny + 1) * c->nzp));
    NK2D_TRY(dev_alloc(c, &c->WT, c->np));
    NK2D_TRY(dev_alloc(c, &c->WB, c->np));
    NK2D_TRY(dev_alloc(c, &c->DZR, (size_t)c->nzp));
    NK2D_TRY(dev_alloc(c, &c->ZM0, (size_t)c->nzp));
    NK2D_TRY(dev_alloc(c, &c->ZM1, (size_t)c->nzp));
    NK2D_TRY(dev_alloc(c, &c->DM, (size_t)c->nzp));
    NK2D_TRY(dev_alloc(c, &c->DMR, (size_t)c->nzp));
    NK2D_TRY(dev_alloc(c, &c->DYR, (size_t)ny));
    NK2D_TRY(dev_alloc(c, &c->BLDMAX, (size_t)ny));
    NK2D_TRY(dev_alloc(c, &c->MASK, c->np));
    NK2D_TRY(dev_alloc(c, &c->WN, c->np));
    NK2D_TRY(dev_alloc(c, &c->JL, c->np));
    NK2D_TRY(dev_alloc(c, &c->JU, c->np));
    NK2D_TRY(dev_alloc(c, &c->JS, c->np));
    NK2D_TRY(dev_alloc(c, &c->JN, c->np));
    NK2D_TRY(dev_alloc(c, &c->JC, c->np));
    NK2D_TRY(dev_alloc(c, &c->LIGHT, c->np));
    NK2D_TRY(dev_alloc(c, &c->UPR, c->np));
    c->YLIN = nullptr;
    c->ylin_set = 0;
    for (int i = 0; i < 5; ++i) NK2D_TRY(dev_alloc(c, &c->KV[i], c->kv_len));
    for (int i = 0; i < 3; ++i) NK2D_TRY(dev_alloc(c, &c->KVN[i], c->kv_len));
    for (int i = 0; i < 5; ++i) NK2D_TRY(dev_alloc(c, &c->JB[i], c->np));
    NK2D_TRY(dev_alloc(c, &c->Y, c->nv));
    NK2D_TRY(dev_alloc(c, &c->YOLD, c->nv));
    NK2D_TRY(dev_alloc(c, &c->F, c->nv));
    NK2D_TRY(dev_alloc(c, &c->Z, 3 * c->nv));
    NK2D_TRY(dev_alloc(c, &c->ZP, 3 * c->nv));
    NK2D_TRY(dev_alloc(c, &c->ZN, 3 * c->nv));
    c->single_swap = 0;
    c->min_sweeps = 1;
    c->team = nk2d_team_auto(c);
    c->jac_stage = 1;     // ONE set of defaults (round 3): the mode the engines and bench.py run; -1 = SciPy's step start
    c->final_fuse = 1;
    c->jac_stage_state = 1;
    c->part_cur = nullptr;
    NK2D_TRY(dev_alloc(c, &c->W, 3 * c->nv));
    NK2D_TRY(dev_alloc(c, &c->BR, c->nv));
    NK2D_TRY(dev_alloc(c, &c->BCR, c->nv));
    NK2D_TRY(dev_alloc(c, &c->BCI, c->nv));
    for (int i = 0; i < 2; ++i) {
        NK2D_TRY(dev_alloc(c, &c->XR[i], c->nv));
        NK2D_TRY(dev_alloc(c, &c->XCR[i], c->nv));
        NK2D_TRY(dev_alloc(c, &c->XCI[i], c->nv));
    }
    NK2D_TRY(dev_alloc(c, &c->FR_INV, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FC_INVR, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FC_INVI, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FR_TAB, (size_t)c->ncol * 14 * 64));
    NK2D_TRY(dev_alloc(c, &c->FC_TABR, (size_t)c->ncol * 14 * 64));
    NK2D_TRY(dev_alloc(c, &c->FC_TABI, (size_t)c->ncol * 14 * 64));
    NK2D_TRY(dev_alloc(c, &c->FR32_INV, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FC32_INVR, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FC32_INVI, c->nv));
    NK2D_TRY(dev_alloc(c, &c->FR32_TAB, (size_t)c->ncol * 14 * 64));
    NK2D_TRY(dev_alloc(c, &c->FC32_TABR, (size_t)c->ncol * 14 * 64));
    NK2D_TRY(dev_alloc(c, &c->FC32_TABI, (size_t)c->ncol * 14 * 64));
    c->factor_fp32 = 0;
    NK2D_TRY(dev_alloc(c, &c->TMP, c->nv));
    NK2D_TRY(dev_alloc(c, &c->TMP2, c->nv));
    NK2D_TRY(dev_alloc(c, &c->PART, (size_t)c->ncol));
    NK2D_TRY(dev_alloc(c, &c->PART2, (size_t)c->ncol));
    NK2D_TRY(dev_alloc(c, &c->STEP_NORM, (size_t)3 * NK2D_OWN_REC_CAP));
    c->frozen_fallbacks = 0;
    c->frozen_resumes = 0;
    c->frozen_cache = nullptr;
    c->frozen_persistent = 1;
    c->frozen_persistent_max_e = 8;
    c->frozen_cache_max_gb = 128.0;
    c->frozen_cache_builds = c->frozen_persistent_years = 0;
    c->frozen_team = 1;
    c->frozen_cache_after = 0;
    c->frozen_cache_pieces = 0;
    c->frozen_cache_piece_mb = 1024.0;
    c->frozen_cache_piece_rows = 0;
    c->frozen_cache_early = 0;
    c->frozen_cache_lean = 0;
    c->frozen_lean_years = 0;
    c->frozen_lean_mem_key = 0;
    c->frozen_forced = 0;
    c->frozen_forced_years = 0;
    c->frozen_phosphorus = 0;
    c->frozen_phosphorus_shallow = 0;
    c->frozen_phosphorus_shallow_years = 0;
    c->frozen_two_waves_last = 0;
    c->frozen_phosphorus_years = c->frozen_two_waves_years = 0;
    c->frozen_cache_piece_allocs = c->frozen_cache_early_requests = 0;
    c->frozen_coef_lds = 63;
    c->frozen_lds_bits = 0;
    c->frozen_early = NK2D_FROZEN_EARLY_DEFAULT;
    c->frozen_early_bits = 0;
    c->frozen_stage_exchange = NK2D_FROZEN_STAGE_EXCHANGE_DEFAULT;
    c->frozen_stage_exchange_bits = 0;
    c->frozen_xlane = NK2D_FROZEN_XLANE_DEFAULT;
    c->frozen_xlane_bits = 0;
    c->frozen_dedicated = NK2D_FROZEN_DEDICATED_DEFAULT;
    c->frozen_dedicated_bits = 0;
    c->frozen_dedicated_years = 0;
    c->stream_xlane = 0;
    c->stream_xlane_bits = 0;
    c->frozen_by_column = 1;
    c->strm = nullptr;
    c->spec_bias = 1.0;
    // (on: taken only where it lets more columns be resident, see stream_alloc)
    c->stream_two_waves = std::getenv("NK2D_STREAM_TWO_WAVES") ? std::atoi(std::getenv("NK2D_STREAM_TWO_WAVES")) : 1;
    c->stream_years = 1;      // free-running years as command streams where eligible (bit 2: frozen years too)
    c->stream_on = 0;
    c->stream_lost = 0;
    c->stream_cmds = c->stream_launches = c->stream_timeouts = c->stream_years_run = 0;
    c->frozen_tape = 0;
    c->tape = nullptr;
    c->tape_rec = c->tape_foreign = 0;
    c->tape_years_run = c->tape_builds = c->tape_timeouts = c->tape_fallbacks = 0;
    c->frozen_wpb = 2;
    c->frozen_alloc_async = 1;
    c->barrier_timeout_ms = 2000.0;
    c->year_fences = 0;
    c->frozen_err_check = NK2D_CKPT_EVERY;   // the rows that start a checkpoint interval: the step before ends in a launch of its own anyway
    c->STEP_PART = nullptr;
    c->step_part_rows = 0;
    NK2D_TRY(dev_alloc(c, &c->RED, (size_t)4096));
    for (int i = 0; i < 8; ++i) NK2D_CHECK(c, hipEventCreateWithFlags(&c->snap_ev[i], hipEventDisableTiming));
    c->snap_ready = 1;
    c->jac_fresh = 1;     // (0 = SciPy's reuse heuristic)
    c->growth_cap = 0.0;
    c->hist_n = 0;
    c->hist_next = 0;
    c->hist_t = nullptr;
    c->hist_host = nullptr;
    c->stream_hist = 0;
    c->stream_hist_mb = 256.0;
    c->HISTBUF = nullptr;
    c->hist_slots = c->hist_buf_elems = 0;
    c->hist_year_samples = c->hist_year_drains = 0;
    c->stream_hist_samples = c->stream_hist_drains = 0;
    c->sweep_wpb = 4;
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hRED, sizeof(double) * 4096));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hPART, sizeof(double) * c->ncol));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hPART2, sizeof(double) * c->ncol));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hPARTB, sizeof(double) * c->ncol));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hPARTC, sizeof(double) * c->ncol));
    c->part_on_host = 0;
    c->speculate = 1;
    c->hook_spec_depth = 2;
    c->factor_pending = 0;
    c->lu_cre = c->lu_ccr = c->lu_cci = 0.0;
    c->rcoef_elems = 0;
    c->RCOEF = nullptr;
    c->hRCOEF = nullptr;

    // ---- axis metrics exactly as SpatialAxis derives them (spatial_axis.py:35-39)
    std::vector<double> zmid(nz), dz(nz), dzr(nz), dzm(nz), dzmr(nz), zm1(nz), dy(ny), dyr(ny);
    for (int k = 0; k < nz; ++k) {
        zmid[k] = 0.5 * (desc->depth_edges[k] + desc->depth_edges[k + 1]);
        dz[k] = desc->depth_edges[k + 1] - desc->depth_edges[k];
        dzr[k] = 1.0 / dz[k];
    }
    for (int k = 0; k < nz; ++k) {
        zm1[k] = (k < nz - 1) ? zmid[k + 1] : 0.0;
        dzm[k] = (k < nz - 1) ? zmid[k + 1] - zmid[k] : 0.0;
        dzmr[k] = (k < nz - 1) ? 1.0 / dzm[k] : 0.0;
    }
    for (int j = 0; j < ny; ++j) {
        dy[j] = desc->ypos_edges[j + 1] - desc->ypos_edges[j];
        dyr[j] = 1.0 / dy[j];
    }
    NK2D_TRY(upload_plane(c, desc->vvel, nz, ny + 1, c->VV));
    {
        std::vector<double> khf((size_t)nz * (ny + 1), 0.0);
        for (int k = 0; k < nz; ++k)
            for (int jf = 1; jf < ny; ++jf) khf[(size_t)k * (ny + 1) + jf] = desc->hmix_coeff[(size_t)k * (ny - 1) + jf - 1];
        NK2D_TRY(upload_plane(c, khf.data(), nz, ny + 1, c->KH));
    }
    NK2D_TRY(upload_plane(c, desc->wvel, nz, ny, c->WT));
    NK2D_TRY(upload_plane(c, desc->wvel + ny, nz, ny, c->WB));
    NK2D_TRY(upload_plane(c, dzr.data(), nz, 1, c->DZR));
    NK2D_TRY(upload_plane(c, zmid.data(), nz, 1, c->ZM0));
    NK2D_TRY(upload_plane(c, zm1.data(), nz, 1, c->ZM1));
    NK2D_TRY(upload_plane(c, dzm.data(), nz, 1, c->DM));
    NK2D_TRY(upload_plane(c, dzmr.data(), nz, 1, c->DMR));
    NK2D_CHECK(c, hipMemcpy(c->DYR, dyr.data(), sizeof(double) * ny, hipMemcpyHostToDevice));
    NK2D_CHECK(c, hipMemcpy(c->BLDMAX, desc->bldepth_max, sizeof(double) * ny, hipMemcpyHostToDevice));
    if (c->kind == 1) NK2D_TRY(upload_plane(c, desc->light_lim, nz, ny, c->LIGHT));
    if (c->kind == 2) {
        if (desc->sms_nrec > 0) {
            NK2D_TRY(dev_alloc(c, &c->SMSREC, (size_t)desc->sms_nrec * c->np));
            for (int r = 0; r < desc->sms_nrec; ++r)
                NK2D_TRY(upload_plane(c, desc->sms_vals + (size_t)r * nz * ny, nz, ny, c->SMSREC + (size_t)r * c->np));
            c->sms_t = new double[desc->sms_nrec];
            std::memcpy(c->sms_t, desc->sms_times, sizeof(double) * desc->sms_nrec);
        }
        if (desc->restore_nrec > 0) {
            NK2D_TRY(dev_alloc(c, &c->RESTREC, (size_t)desc->restore_nrec * ny));
            NK2D_CHECK(c, hipMemcpy(c->RESTREC, desc->restore_vals, sizeof(double) * desc->restore_nrec * ny, hipMemcpyHostToDevice));
            c->rest_t = new double[desc->restore_nrec];
            std::memcpy(c->rest_t, desc->restore_times, sizeof(double) * desc->restore_nrec);
        }
    }
    build_front(c, dzr, dyr);
    // the descriptor's pointers are not kept
    c->d.depth_edges = c->d.ypos_edges = c->d.vvel = c->d.wvel = c->d.hmix_coeff = c->d.bldepth_max = nullptr;
    c->d.light_lim = nullptr;
    c->d.restore_times = c->d.restore_vals = c->d.sms_times = c->d.sms_vals = nullptr;
    // default region: everything in region 1 with unit weights until nk2d_set_region is called
    {
        std::vector<int32_t> m((size_t)nz * ny, 1);
        std::vector<double> w((size_t)nz * ny, 1.0);
        NK2D_TRY(nk2d_set_region(c, m.data(), w.data(), 1));
    }
    return 0;
}

extern "C" int nk2d_create(const nk2d_desc* desc, nk2d_ctx** out) {
    if (!desc || !out) return -2;
    nk2d_ctx* c = new (std::nothrow) nk2d_ctx();
    if (!c) return -2;
    c->stream_ = nullptr;
    c->STAGE = nullptr;
    c->hSTAGE = nullptr;
    c->stage_elems = 0;
    c->dl_pool = nullptr;
    c->precond = nullptr;
    c->pc_valu = 0;
    c->pc_fused = 1;
    c->pc_fp32 = 0;
    c->pc_refine = 1;
    c->pc_two_ended = 0;
    c->pc_setup_rounds = c->pc_sub_launches = 0;
    c->pc_phos_applies = 0;
    c->pc_pivot_wave = 0;
    c->pc_pivot_wave_steps = 0;
    c->pc_panel = 32;
    c->pc_panel_steps = 0;
    c->st = nk2d_stats();
    c->prof_every = 0;
    c->snap_ready = 0;
    c->prof_used = 0;
    c->prof_ms_sum = 0.0;
    c->prof_overhead_ms = 0.0;
    c->prof_cnt = 0;
    c->prof_windows = 0;
    c->win_open = 0;
    c->win_seq = 0;
    c->sweep_launches = 0;
    c->sweep_bytes = 0.0;
    c->fused_bytes_all = 0.0;
    c->norm_hook = nullptr;
    c->norm_hook_user = nullptr;
    c->norm_hook_vec = nullptr;
    c->norm_hook_vec_user = nullptr;
    c->global_n = 0.0;
    c->timer_ready = 0;
    c->YR_PART = c->YR_OUT = c->hYR_OUT = c->YR_REC = nullptr;
    c->YR_SYNC = nullptr;
    c->YR_MTAB = nullptr;
    *out = c;  // returned even on failure so that nk2d_last_error can be read
    return create_impl(c, desc);
}

extern "C" void nk2d_destroy(nk2d_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    nk2d_stream_free(c);
    if (c->stream_) (void)hipStreamSynchronize(c->stream_);
    nk2d_precond_free(c);
    nk2d_frozen_cache_free(c);
    double* bufs[] = {c->VV, c->KH, c->WT, c->WB, c->DZR, c->ZM0, c->ZM1, c->DM, c->DMR, c->DYR, c->BLDMAX, c->WN,
                      c->JL, c->JU, c->JS, c->JN, c->JC, c->KV[0], c->KV[1], c->KV[2], c->KV[3], c->KV[4], c->KVN[0], c->KVN[1], c->KVN[2], c->JB[0], c->JB[1],
                      c->JB[2], c->JB[3], c->JB[4], c->Y,
                      c->YOLD, c->F, c->Z, c->ZP, c->ZN, c->ZS, c->W, c->BR, c->BCR, c->BCI, c->XR[0], c->XR[1], c->XCR[0],
                      c->XCR[1], c->XCI[0], c->XCI[1], c->TMP, c->TMP2, c->PART, c->PART2, c->STEP_NORM, c->STEP_PART, c->RED, c->STAGE, c->RCOEF,
                      c->FR_INV, c->FC_INVR, c->FC_INVI, c->FR_TAB, c->FC_TABR, c->FC_TABI,
                      c->LIGHT, c->UPR, c->YLIN,
                      c->SMSREC, c->RESTREC, c->HISTBUF};
    for (double* b : bufs)
        if (b) (void)hipFree(b);
    delete[] c->sms_t;
    delete[] c->rest_t;
    for (double* b : c->vec_pool) (void)hipFree(b);
    for (double* b : c->ckpt) (void)hipFree(b);
    float* fbufs[] = {c->FR32_INV, c->FC32_INVR, c->FC32_INVI, c->FR32_TAB, c->FC32_TABR, c->FC32_TABI};
    for (float* b : fbufs)
        if (b) (void)hipFree(b);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->timer_ready) { (void)hipEventDestroy(c->timer_ev[0]); (void)hipEventDestroy(c->timer_ev[1]); }
    if (c->YR_OUT) {
        (void)hipFree(c->YR_PART); (void)hipFree(c->YR_OUT); (void)hipFree(c->YR_SYNC); (void)hipFree(c->YR_MTAB);
        if (c->YR_REC) (void)hipFree(c->YR_REC);
        (void)hipHostFree(c->hYR_OUT);
        (void)hipEventDestroy(c->yr_ev[0]); (void)hipEventDestroy(c->yr_ev[1]);
    }
    if (c->MASK) (void)hipFree(c->MASK);
    if (c->hRED) (void)hipHostFree(c->hRED);
    if (c->hPART) (void)hipHostFree(c->hPART);
    if (c->hPART2) (void)hipHostFree(c->hPART2);
    if (c->hPARTB) (void)hipHostFree(c->hPARTB);
    if (c->hPARTC) (void)hipHostFree(c->hPARTC);
    if (c->hSTAGE) (void)hipHostFree(c->hSTAGE);
    download_pool_free(c);
    if (c->hRCOEF) (void)hipHostFree(c->hRCOEF);
    if (c->snap_ready) {
        for (int i = 0; i < 8; ++i) (void)hipEventDestroy(c->snap_ev[i]);
    }
    if (c->stream_) (void)hipStreamDestroy(c->stream_);
    delete c;
}

// ---------------------------------------------------------------------------------
// regions
// ---------------------------------------------------------------------------------
__global__ void k_to_int(const double* __restrict__ src, int32_t* __restrict__ dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (int32_t)src[i];
}

extern "C" int nk2d_set_region(nk2d_ctx* c, const int32_t* mask, const double* weight, int32_t nreg) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (nreg < 1) return nk2d_fail(c, "nk2d_set_region: nreg < 1");
    const size_t P = (size_t)c->nz * c->ny;
    // rows of the region mean matrix: w / sum_region(w), summed in flat index order
    // (model_config.py:292-315)
    std::vector<double> wn(P, 0.0), mk(P, 0.0);
    for (int r = 1; r <= nreg; ++r) {
        double sum = 0.0;
        for (size_t i = 0; i < P; ++i)
            if (mask[i] == r) sum += weight[i];
        const double sum_r = 1.0 / sum;
        for (size_t i = 0; i < P; ++i)
            if (mask[i] == r) wn[i] = sum_r * weight[i];
    }
    for (size_t i = 0; i < P; ++i) {
        if (mask[i] > nreg) return nk2d_fail(c, "nk2d_set_region: mask value exceeds nreg");
        mk[i] = (double)mask[i];
    }
    NK2D_TRY(upload_plane(c, wn.data(), c->nz, c->ny, c->WN));
    NK2D_TRY(upload_plane(c, mk.data(), c->nz, c->ny, c->TMP));  // TMP has at least np elements
    hipLaunchKernelGGL(k_to_int, dim3((unsigned)((c->np + 255) / 256)), dim3(256), 0, nk2d_s(c), c->TMP, c->MASK, c->np);
    NK2D_CHECK(c, hipGetLastError());
    if (nreg != c->nreg) {
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        nk2d_tape_forget(c);     // (the commands of a recorded frozen year write norm partials to PART)
        NK2D_CHECK(c, hipFree(c->PART));
        c->PART = nullptr;
        NK2D_TRY(dev_alloc(c, &c->PART, (size_t)c->ncol * nreg));
        if (c->RCOEF) NK2D_CHECK(c, hipFree(c->RCOEF));
        if (c->hRCOEF) NK2D_CHECK(c, hipHostFree(c->hRCOEF));
        c->RCOEF = c->hRCOEF = nullptr;
        c->rcoef_elems = (size_t)nreg * 1024 + 4096;
        NK2D_TRY(dev_alloc(c, &c->RCOEF, c->rcoef_elems));
        NK2D_CHECK(c, hipHostMalloc((void**)&c->hRCOEF, sizeof(double) * c->rcoef_elems));
        if ((size_t)nreg * 2 > 4096) return nk2d_fail(c, "nk2d_set_region: too many regions");
    }
    c->nreg = nreg;
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}

// ---------------------------------------------------------------------------------
// vectors
// ---------------------------------------------------------------------------------
// State vectors come from a per-context pool: hipMalloc / hipFree cost milliseconds each and the
// solver mirrors create and drop a dozen temporaries per Krylov iteration.  A vector handed out
// is zero-filled (stream ordered); freed vectors are kept (at most NK2D_POOL_MAX) until destroy.
#define NK2D_POOL_MAX 64
extern "C" int nk2d_vec_alloc(nk2d_ctx* c, nk2d_vec* out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    double* p = nullptr;
    {
        // handles may be released from another host thread (garbage collection of the caller)
        std::lock_guard<std::mutex> lock(c->pool_mutex);
        if (!c->vec_pool.empty()) {
            p = c->vec_pool.back();
            c->vec_pool.pop_back();
        }
    }
    if (p) {
        NK2D_CHECK(c, hipMemsetAsync(p, 0, sizeof(double) * c->nv, nk2d_s(c)));
    } else {
        NK2D_TRY(dev_alloc(c, &p, c->nv));
    }
    *out = p;
    return 0;
}
extern "C" int nk2d_vec_free(nk2d_ctx* c, nk2d_vec v) {
    if (!v) return 0;
    NK2D_CHECK(c, hipSetDevice(c->dev));
    {
        std::lock_guard<std::mutex> lock(c->pool_mutex);
        if (c->vec_pool.size() < NK2D_POOL_MAX) {
            // work queued on the context's stream that still reads v finishes before any later use,
            // which is queued on the same stream
            c->vec_pool.push_back((double*)v);
            return 0;
        }
    }
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    NK2D_CHECK(c, hipFree(v));
    return 0;
}
extern "C" int nk2d_vec_upload(nk2d_ctx* c, nk2d_vec v, const double* host) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    const size_t n = (size_t)c->tc * c->nz * c->ny;
    NK2D_TRY(stage_in(c, host, n));
    NK2D_TRY(nk2d_k_pack_state(c, c->STAGE, (double*)v));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}
extern "C" int nk2d_vec_download(nk2d_ctx* c, nk2d_vec v, double* host) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    const size_t n = (size_t)c->tc * c->nz * c->ny;
    NK2D_TRY(ensure_stage(c, n));
    NK2D_TRY(nk2d_k_unpack_state(c, (const double*)v, c->STAGE));
    return stage_out(c, host, n);
}
// A download in two halves, for a caller that writes the values to a file on a thread of its own (the checkpoint trail,
// newton-krylov_ooc_amd/trail.py): `begin` queues the layout conversion and the copy into a pinned buffer of the
// download's OWN behind whatever the context's stream holds and returns at once -- what is launched on the stream
// afterwards (the next forward year) does not wait for the host, and may change `v`: the conversion has read it by then in
// stream order --; `end`, on ANY host thread, waits for that copy alone (an event, not the stream) and hands the values
// out.  `end` touches nothing of the context but the pool of staging pairs, under the pool's mutex.
extern "C" int nk2d_vec_download_begin(nk2d_ctx* c, nk2d_vec v, void** ticket) {
    if (!ticket) return nk2d_fail(c, "nk2d_vec_download_begin: null ticket");
    NK2D_CHECK(c, hipSetDevice(c->dev));
    const size_t n = (size_t)c->tc * c->nz * c->ny;
    if (!c->dl_pool) c->dl_pool = new nk2d_download_pool();
    nk2d_download* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->dl_pool->m);
        if (!c->dl_pool->idle.empty()) { t = c->dl_pool->idle.back(); c->dl_pool->idle.pop_back(); }
    }
    if (!t) {
        t = new nk2d_download();
        hipError_t rc = hipMalloc((void**)&t->dev, sizeof(double) * n);
        if (rc == hipSuccess) rc = hipHostMalloc((void**)&t->host, sizeof(double) * n);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&t->done, hipEventDisableTiming);
        if (rc != hipSuccess) {
            if (t->dev) (void)hipFree(t->dev);
            if (t->host) (void)hipHostFree(t->host);
            delete t;
            NK2D_CHECK(c, rc);
        }
        t->n = n;
        std::lock_guard<std::mutex> lk(c->dl_pool->m);
        c->dl_pool->all.push_back(t);
    }
    int rc = nk2d_k_unpack_state(c, (const double*)v, t->dev);
    if (rc == 0 && hipMemcpyAsync(t->host, t->dev, sizeof(double) * n, hipMemcpyDeviceToHost, nk2d_s(c)) != hipSuccess)
        rc = nk2d_fail(c, "nk2d_vec_download_begin: the copy to the host could not be queued");
    if (rc == 0 && hipEventRecord(t->done, nk2d_s(c)) != hipSuccess) rc = nk2d_fail(c, "nk2d_vec_download_begin: hipEventRecord failed");
    if (rc != 0) {      // (the staging pair goes back to the pool: no ticket was handed out)
        std::lock_guard<std::mutex> lk(c->dl_pool->m);
        c->dl_pool->idle.push_back(t);
        return rc;
    }
    *ticket = t;
    return 0;
}
extern "C" int nk2d_vec_download_end(nk2d_ctx* c, void* ticket, double* host) {
    nk2d_download* t = (nk2d_download*)ticket;
    if (!c || !c->dl_pool || !t) return -2;
    (void)hipSetDevice(c->dev);
    const hipError_t rc = hipEventSynchronize(t->done);
    if (rc == hipSuccess && host) std::memcpy(host, t->host, sizeof(double) * t->n);
    {
        std::lock_guard<std::mutex> lk(c->dl_pool->m);
        c->dl_pool->idle.push_back(t);
    }
    return rc == hipSuccess ? 0 : -1;
}
extern "C" int nk2d_vec_copy(nk2d_ctx* c, nk2d_vec dst, nk2d_vec src) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipMemcpyAsync(dst, src, sizeof(double) * c->nv, hipMemcpyDeviceToDevice, nk2d_s(c)));
    return 0;
}
extern "C" int nk2d_vec_zero(nk2d_ctx* c, nk2d_vec v) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_CHECK(c, hipMemsetAsync(v, 0, sizeof(double) * c->nv, nk2d_s(c)));
    return 0;
}

// ---------------------------------------------------------------------------------
// deterministic model kernels
// ---------------------------------------------------------------------------------
extern "C" int nk2d_tend(nk2d_ctx* c, double t, nk2d_vec y, nk2d_vec f) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    double* out[1] = {c->KV[4]};
    NK2D_TRY(nk2d_k_vmix(c, 1, &t, out));
    NK2D_TRY(nk2d_k_tend(c, (const double*)y, c->KV[4], (double*)f));
    return 0;
}

extern "C" int nk2d_vmix_coeff(nk2d_ctx* c, double t, double* host_out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    double* out[1] = {c->KV[4]};
    NK2D_TRY(nk2d_k_vmix(c, 1, &t, out));
    const size_t n = (size_t)(c->nz - 1) * c->ny;
    NK2D_TRY(ensure_stage(c, n));
    NK2D_TRY(nk2d_k_unpack_plane(c, c->KV[4], c->nz - 1, c->ny, c->STAGE));
    return stage_out(c, host_out, n);
}

// linearisation state of the stand-alone Jacobian entry points (state dependent modules only)
static const double* lin_state(nk2d_ctx* c) { return (c->kind != 0 && c->ylin_set) ? c->YLIN : nullptr; }

extern "C" int nk2d_set_lin_state(nk2d_ctx* c, nk2d_vec y) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (!c->YLIN) NK2D_TRY(dev_alloc(c, &c->YLIN, c->nv));
    NK2D_CHECK(c, hipMemcpyAsync(c->YLIN, y, sizeof(double) * c->nv, hipMemcpyDeviceToDevice, nk2d_s(c)));
    c->ylin_set = 1;
    return 0;
}

extern "C" int nk2d_jacobian_apply(nk2d_ctx* c, double t, nk2d_vec v, nk2d_vec out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    double* kv[1] = {c->KV[4]};
    NK2D_TRY(nk2d_k_vmix(c, 1, &t, kv));
    NK2D_TRY(nk2d_k_jac(c, c->KV[4], lin_state(c)));
    NK2D_TRY(nk2d_k_jac_apply(c, (const double*)v, (double*)out));
    return 0;
}

extern "C" int nk2d_jacobian_diags(nk2d_ctx* c, double t, double* host_out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (c->kind == 1) return nk2d_fail(c, "nk2d_jacobian_diags: the phosphorus Jacobian is not five diagonals; use nk2d_jacobian_apply");
    double* out[1] = {c->KV[4]};
    NK2D_TRY(nk2d_k_vmix(c, 1, &t, out));
    NK2D_TRY(nk2d_k_jac(c, c->KV[4], lin_state(c)));
    const size_t P = (size_t)c->nz * c->ny;
    NK2D_TRY(ensure_stage(c, P));
    const double* planes[5] = {c->JL, c->JS, c->JC, c->JN, c->JU};
    std::vector<double> tmp(P), extra;
    if (c->kind == 2) {
        // state dependent part of the diagonal (sink threshold, forced.py:188-202); zero without it
        extra.resize(P);
        NK2D_TRY(nk2d_k_unpack_plane(c, c->UPR, c->nz, c->ny, c->STAGE));
        NK2D_TRY(stage_out(c, extra.data(), P));
    }
    for (int d = 0; d < 5; ++d) {
        NK2D_TRY(nk2d_k_unpack_plane(c, planes[d], c->nz, c->ny, c->STAGE));
        NK2D_TRY(stage_out(c, tmp.data(), P));
        for (int tr = 0; tr < c->tc; ++tr) {
            double* dst = host_out + ((size_t)d * c->tc + tr) * P;
            std::memcpy(dst, tmp.data(), sizeof(double) * P);
            if (d == 2) {
                // module part of the diagonal (iage.py:55-64)
                for (int j = 0; j < c->ny; ++j) dst[j] = dst[j] + (-c->d.surf_rate[tr]);
                if (c->d.decay_rate[tr] != 0.0)
                    for (size_t i = 0; i < P; ++i) dst[i] = dst[i] + (-c->d.decay_rate[tr]);
                if (!extra.empty())
                    for (size_t i = 0; i < P; ++i) dst[i] = dst[i] - extra[i];
            }
        }
    }
    return 0;
}

extern "C" int nk2d_shifted_solve(nk2d_ctx* c, double t_jac, double h, double mu_re, double mu_im, nk2d_vec b_re,
                                  nk2d_vec b_im, nk2d_vec x_re, nk2d_vec x_im, int32_t* sweeps_out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    double* out[1] = {c->KV[4]};
    NK2D_TRY(nk2d_k_vmix(c, 1, &t_jac, out));
    NK2D_TRY(nk2d_k_jac(c, c->KV[4], lin_state(c)));
    const bool cplxsys = mu_im != 0.0;
    const int m = nk2d_sweeps_for(c, mu_re / h);
    NK2D_TRY(nk2d_k_factor(c, !cplxsys, cplxsys, mu_re / h, mu_re / h, mu_im / h));
    int src = 0;
    for (int it = 0; it < m; ++it) {
        NK2D_TRY(nk2d_k_sweep(c, !cplxsys, cplxsys, it == 0, mu_re / h, mu_re / h, mu_im / h, (const double*)b_re,
                              (const double*)b_re, (const double*)b_im, src));
        src = 1 - src;
    }
    if (!cplxsys) {
        NK2D_CHECK(c, hipMemcpyAsync(x_re, c->XR[src], sizeof(double) * c->nv, hipMemcpyDeviceToDevice, nk2d_s(c)));
    } else {
        NK2D_CHECK(c, hipMemcpyAsync(x_re, c->XCR[src], sizeof(double) * c->nv, hipMemcpyDeviceToDevice, nk2d_s(c)));
        NK2D_CHECK(c, hipMemcpyAsync(x_im, c->XCI[src], sizeof(double) * c->nv, hipMemcpyDeviceToDevice, nk2d_s(c)));
    }
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    if (sweeps_out) *sweeps_out = m;
    return 0;
}

extern "C" int nk2d_comp_fcn(nk2d_ctx* c, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, const double* replay,
                             int64_t replay_n, double* record, int64_t record_cap, int64_t* record_n) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (record_n) *record_n = 0;
    const int rc = nk2d_radau_year(c, x, fx, stats, replay, replay_n, record, record_cap, record_n);
    // option "frozen_cache_early" (with "frozen_cache_pieces"): the pieces of the schedule this year recorded are asked for now
    if (rc == 0 && record && record_n && *record_n > 0 && c->frozen_cache_pieces && c->frozen_cache_early)
        NK2D_TRY(nk2d_frozen_cache_early(c, record, *record_n));
    return rc;
}

// forward year on a schedule this library recorded itself (nk2d_comp_fcn with `record`) under the same options: the
// steps, Newton iteration counts, Jacobian times and factorisations of the recorded year with its own inner tolerance
// and no decision taken -- for x itself the recorded year again, bit for bit; for x + sigma v the same discrete map
extern "C" int nk2d_comp_fcn_frozen(nk2d_ctx* c, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, const double* sched,
                                    int64_t sched_n) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (!sched || sched_n < 1) return nk2d_fail(c, "nk2d_comp_fcn_frozen: empty schedule");
    return nk2d_radau_year(c, x, fx, stats, sched, sched_n, nullptr, 0, nullptr, true);
}

extern "C" int nk2d_frozen_fallbacks(nk2d_ctx* c, int64_t* n) {
    if (n) *n = c->frozen_fallbacks;
    return 0;
}

extern "C" int nk2d_frozen_resumes(nk2d_ctx* c, int64_t* n) {
    if (n) *n = c->frozen_resumes;
    return 0;
}

extern "C" int nk2d_get_counter(nk2d_ctx* c, const char* name, int64_t* out) {
    const std::string key(name ? name : "");
    int64_t v = 0;
    if (key == "frozen_persistent_years") v = c->frozen_persistent_years;
    else if (key == "frozen_cache_builds") v = c->frozen_cache_builds;
    else if (key == "frozen_team_years") v = c->frozen_team_years;
    else if (key == "stream_years_run") v = c->stream_years_run;
    else if (key == "stream_commands") v = c->stream_cmds;
    else if (key == "stream_launches") v = c->stream_launches;
    else if (key == "stream_timeouts") v = c->stream_timeouts;
    else if (key == "stream_columns_per_workgroup") v = nk2d_stream_columns_per_workgroup(c);
    else if (key == "stream_two_waves_kernel") v = nk2d_stream_two_waves(c);
    else if (key == "stream_hist_samples") v = c->stream_hist_samples;
    else if (key == "stream_hist_drains") v = c->stream_hist_drains;
    else if (key == "pc_setup_rounds") v = c->pc_setup_rounds;
    else if (key == "pc_sub_launches") v = c->pc_sub_launches;
    else if (key == "pc_pivot_wave_steps") v = c->pc_pivot_wave_steps;
    else if (key == "pc_panel_steps") v = c->pc_panel_steps;
    else if (key == "pc_phos_applies") v = c->pc_phos_applies;
    else if (key == "tape_years_run") v = c->tape_years_run;
    else if (key == "tape_builds") v = c->tape_builds;
    else if (key == "tape_timeouts") v = c->tape_timeouts;
    else if (key == "tape_fallbacks") v = c->tape_fallbacks;
    else if (key == "tape_bytes") v = nk2d_tape_size(c, 0);
    else if (key == "tape_commands") v = nk2d_tape_size(c, 1);
    else if (key.rfind("stream_prof_", 0) == 0) {
        // stream_prof_0 .. stream_prof_11: see nk2d_stream_profile
        double pr[12];
        NK2D_TRY(nk2d_stream_profile(c, pr));
        const int i = std::atoi(key.c_str() + 12);
        v = (i >= 0 && i < 12) ? (int64_t)pr[i] : 0;
    }
    else if (key.rfind("xlane_selftest_", 0) == 0) {
        // xlane_selftest_<w>_<row>_<lane>: see xlane_selftest_run
        int w = -1, row = -1, lane = -1;
        if (std::sscanf(key.c_str() + 15, "%d_%d_%d", &w, &row, &lane) != 3 || w < 0 || w > 1 || row < 0 || row >= NK2D_XLANE_SELFTEST_ROWS ||
            lane < 0 || lane > 63)
            return nk2d_fail(c, "nk2d_get_counter: unknown counter " + key);
        v = xl_selftest_out[((size_t)w * NK2D_XLANE_SELFTEST_ROWS + row) * 64 + lane];
    }
    else if (key == "frozen_launch_us") v = c->frozen_launch_us;
    else if (key == "frozen_cache_pending") v = nk2d_frozen_cache_pending(c);
    else if (key == "frozen_cache_bytes") v = nk2d_frozen_cache_bytes(c);
    else if (key == "frozen_cache_pieces") v = nk2d_frozen_cache_npieces(c);
    else if (key == "frozen_cache_lean") v = nk2d_frozen_cache_is_lean(c);
    else if (key == "frozen_lds_bits") v = c->frozen_lds_bits;
    else if (key == "frozen_early_bits") v = c->frozen_early_bits;
    else if (key == "frozen_stage_exchange_bits") v = c->frozen_stage_exchange_bits;
    else if (key == "frozen_xlane_bits") v = c->frozen_xlane_bits;
    else if (key == "frozen_dedicated_bits") v = c->frozen_dedicated_bits;
    else if (key == "frozen_dedicated_years") v = c->frozen_dedicated_years;
    else if (key == "stream_xlane_bits") v = c->stream_xlane_bits;
    else if (key == "frozen_step_sums_hash") v = c->frozen_step_sums_hash;
    else if (key == "frozen_lean_years") v = c->frozen_lean_years;
    else if (key == "frozen_forced_years") v = c->frozen_forced_years;
    else if (key == "frozen_phosphorus_years") v = c->frozen_phosphorus_years;
    else if (key == "frozen_phosphorus_shallow_years") v = c->frozen_phosphorus_shallow_years;
    else if (key == "frozen_two_waves_years") v = c->frozen_two_waves_years;
    else if (key == "frozen_cache_piece_allocs") v = nk2d_frozen_cache_piece_allocs(c);
    else if (key == "frozen_cache_early_requests") v = c->frozen_cache_early_requests;
    else if (key == "frozen_fallbacks") v = c->frozen_fallbacks;
    else if (key == "frozen_resumes") v = c->frozen_resumes;
    else if (key == "spec_launches_dropped") v = c->cnt_spec_dropped;
    else if (key == "spec_front_launches_dropped") v = c->cnt_front_dropped;
    else if (key == "err_estimates_queued") v = c->cnt_err_queued;
    else if (key == "err_estimates_dropped") v = c->cnt_err_void;
    else return nk2d_fail(c, "nk2d_get_counter: unknown counter " + key);
    if (out) *out = v;
    return 0;
}

extern "C" int nk2d_schedule_fingerprint(nk2d_ctx* c, double* out) {
    if (out) *out = nk2d_fingerprint(c);
    return 0;
}

extern "C" int nk2d_last_schedule(nk2d_ctx* c, double* out, int64_t cap, int64_t* n) {
    const int64_t rows = (int64_t)(c->last_sched.size() / NK2D_SCHED_WIDTH);
    if (n) *n = rows;
    if (out) {
        if (cap < rows) return nk2d_fail(c, "nk2d_last_schedule: buffer too small", -4);
        std::memcpy(out, c->last_sched.data(), sizeof(double) * c->last_sched.size());
    }
    return 0;
}

extern "C" int nk2d_set_frozen_schedule(nk2d_ctx* c, const double* sched, int64_t sched_n) {
    if (sched_n < 0 || (sched_n > 0 && !sched)) return nk2d_fail(c, "nk2d_set_frozen_schedule: bad arguments");
    c->frozen_sched.assign(sched, sched + (size_t)sched_n * NK2D_SCHED_WIDTH);
    return 0;
}

// samples of the solution at t_eval (scipy ivp.py:707-723: every t_eval <= t not yet emitted is
// evaluated with the dense output of the step just taken)
int nk2d_hist_sample(nk2d_ctx* c, double t_old, double t_new, bool first) {
    const size_t n = (size_t)c->tc * c->nz * c->ny;
    double x = 0.0;
    while (nk2d_hist_due(c, t_old, t_new, &x)) {
        NK2D_TRY(nk2d_r_dense(c, x, c->TMP));
        NK2D_TRY(ensure_stage(c, n));
        NK2D_TRY(nk2d_k_unpack_state(c, c->TMP, c->STAGE));
        NK2D_TRY(stage_out(c, c->hist_host + (size_t)c->hist_next * n, n));
        c->hist_next++;
    }
    (void)first;
    return 0;
}

// ---- option "stream_hist": the samples of a year that runs as a command stream are commands of its resident kernel ----
// The sample buffer: nslots = clamp(floor(stream_hist_mb MiB / (nv 8)), 1, hist_n) packed samples, allocated before the
// first sampled stream year (no kernel is resident then: freeing memory waits for the device), kept, grown when needed.
int nk2d_hist_buf_ready(nk2d_ctx* c) {
    nk2d_hist_buf_reset(c);
    const double bytes = c->stream_hist_mb * 1048576.0;
    const double fit = std::floor(bytes / (8.0 * (double)c->nv));
    c->hist_slots = (size_t)std::min((double)c->hist_n, std::max(1.0, fit));
    const size_t need = c->hist_slots * c->nv;
    if (c->hist_buf_elems < need) {
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        if (c->HISTBUF) NK2D_CHECK(c, hipFree(c->HISTBUF));
        c->HISTBUF = nullptr;
        c->hist_buf_elems = 0;
        NK2D_CHECK(c, hipMalloc((void**)&c->HISTBUF, sizeof(double) * need));
        c->hist_buf_elems = need;
    }
    return ensure_stage(c, (size_t)c->tc * c->nz * c->ny);
}

// a year that starts or is given up (the kernel lost: rerun by launches): nothing buffered, nothing of it booked -- the
// counters take a year's samples and drains when it has run as a stream to its end (nk2d_hist_year_done)
void nk2d_hist_buf_reset(nk2d_ctx* c) {
    c->hist_slot_k.clear();
    c->hist_year_samples = c->hist_year_drains = 0;
}
void nk2d_hist_year_done(nk2d_ctx* c) {
    c->stream_hist_samples += c->hist_year_samples;
    c->stream_hist_drains += c->hist_year_drains;
    c->hist_year_samples = c->hist_year_drains = 0;
}

// every buffered sample, in the order of the slots: unpack -> STAGE -> pinned twin -> the caller's array.  Launches and
// copies on the context's stream, behind the resident kernel (which the first of them tells to finish).
int nk2d_hist_drain(nk2d_ctx* c) {
    if (c->hist_slot_k.empty()) return 0;
    const size_t n = (size_t)c->tc * c->nz * c->ny;
    NK2D_TRY(ensure_stage(c, n));
    for (size_t slot = 0; slot < c->hist_slot_k.size(); ++slot) {
        NK2D_TRY(nk2d_k_unpack_state(c, c->HISTBUF + slot * c->nv, c->STAGE));
        NK2D_TRY(stage_out(c, c->hist_host + (size_t)c->hist_slot_k[slot] * n, n));
    }
    c->hist_year_samples += (int64_t)c->hist_slot_k.size();
    c->hist_year_drains++;
    c->hist_slot_k.clear();
    return 0;
}

// the samples due at t_new, right behind the boundary command of the accepted step (t_old, t_new): after the boundary's
// pointer swaps YOLD is the step's old state and ZP its Z, and nothing writes them before the next boundary
int nk2d_hist_push(nk2d_ctx* c, double t_old, double t_new) {
    double x = 0.0;
    while (nk2d_hist_due(c, t_old, t_new, &x)) {
        if (c->hist_slot_k.size() >= c->hist_slots) NK2D_TRY(nk2d_hist_drain(c));
        NK2D_TRY(nk2d_r_dense_push(c, x, c->HISTBUF + c->hist_slot_k.size() * c->nv));
        c->hist_slot_k.push_back(c->hist_next);
        c->hist_next++;
    }
    return 0;
}

extern "C" int nk2d_comp_fcn_hist(nk2d_ctx* c, nk2d_vec x, nk2d_vec fx, nk2d_stats* stats, int32_t n_eval,
                                  const double* t_eval, double* host_hist) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    for (int i = 1; i < n_eval; ++i)
        if (!(t_eval[i] > t_eval[i - 1])) return nk2d_fail(c, "nk2d_comp_fcn_hist: t_eval must be increasing");
    if (n_eval > 0 && (t_eval[0] < c->d.t0 || t_eval[n_eval - 1] > c->d.t1))
        return nk2d_fail(c, "nk2d_comp_fcn_hist: t_eval outside the time range");
    c->hist_n = n_eval;
    c->hist_next = 0;
    c->hist_t = t_eval;
    c->hist_host = host_hist;
    nk2d_hist_buf_reset(c);
    const int rc = nk2d_radau_year(c, x, fx, stats, nullptr, 0, nullptr, 0, nullptr);
    const bool complete = c->hist_next == n_eval && c->hist_slot_k.empty();
    nk2d_hist_buf_reset(c);
    c->hist_n = 0;
    c->hist_t = nullptr;
    c->hist_host = nullptr;
    if (rc != 0) return rc;
    if (!complete) return nk2d_fail(c, "nk2d_comp_fcn_hist: not every t_eval sample was produced");
    return 0;
}

// ---------------------------------------------------------------------------------
// region-weighted state algebra
// ---------------------------------------------------------------------------------
// value of a per-region scalar at a cell (tracer_module_state_base.py:502-515): fill 1.0
// where the mask is <= 0
__device__ __forceinline__ double bcast(const double* __restrict__ coef, int m) { return (m > 0) ? coef[m - 1] : 1.0; }

template <int E>
__global__ void k_dot(int ncol, int ny, int nreg, const double* __restrict__ a, const double* __restrict__ b,
                      const double* __restrict__ wn, const int32_t* __restrict__ mask, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    double aa[E], bb[E], ww[E];
    int mm[E];
    load_col<E>(a, task, lane, aa);
    load_col<E>(b, task, lane, bb);
    load_col<E>(wn, j, lane, ww);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        mm[e] = mask[(size_t)j * (E * 64) + e * 64 + lane];
        aa[e] = ww[e] * (aa[e] * bb[e]);
    }
    for (int r = 1; r <= nreg; ++r) {
        double acc = 0.0;
        bool any = false;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (mm[e] == r) { acc += aa[e]; any = true; }
        double tot = 0.0;
        if (__any(any)) tot = wave_sum(acc);
        if (lane == 0) part[(size_t)task * nreg + (r - 1)] = tot;
    }
}

// out = bcast(a) x + bcast(b) y ; products first, then the sum
template <int E>
__global__ void k_axpby(int ncol, int ny, const double* __restrict__ ca, const double* __restrict__ x,
                        const double* __restrict__ cb, const double* __restrict__ y, const int32_t* __restrict__ mask,
                        double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    double xx[E], yy[E];
    load_col<E>(x, task, lane, xx);
    load_col<E>(y, task, lane, yy);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int m = mask[(size_t)j * (E * 64) + e * 64 + lane];
        xx[e] = bcast(ca, m) * xx[e] + bcast(cb, m) * yy[e];
    }
    store_col<E>(out, task, lane, xx);
}

// out = bcast(s) * (x - y)   (y may be null: out = bcast(s) * x)
template <int E>
__global__ void k_diff_scale(int ncol, int ny, const double* __restrict__ x, const double* __restrict__ y,
                             const double* __restrict__ cs, const int32_t* __restrict__ mask, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    double xx[E], yy[E];
    load_col<E>(x, task, lane, xx);
    if (y) load_col<E>(y, task, lane, yy);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int m = mask[(size_t)j * (E * 64) + e * 64 + lane];
        const double d = y ? (xx[e] - yy[e]) : xx[e];
        xx[e] = d * bcast(cs, m);
    }
    store_col<E>(out, task, lane, xx);
}

// w -= bcast(h) * v   (one modified Gram-Schmidt projection, model_state_base.py:375-376)
template <int E>
__global__ void k_mgs_update(int ncol, int ny, double* __restrict__ w, const double* __restrict__ v,
                             const double* __restrict__ h, const int32_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    double ww[E], vv[E];
    load_col<E>(w, task, lane, ww);
    load_col<E>(v, task, lane, vv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int m = mask[(size_t)j * (E * 64) + e * 64 + lane];
        ww[e] = ww[e] - bcast(h, m) * vv[e];
    }
    store_col<E>(w, task, lane, ww);
}

// res = c_0 X_0; res += c_j X_j  (model_state_base.py:619-624)
template <int E>
__global__ void k_lin_comb(int ncol, int ny, int n, int nreg, const double* const* __restrict__ vecs,
                           const double* __restrict__ coef, const int32_t* __restrict__ mask, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    int mm[E];
    double acc[E], xx[E];
#pragma unroll
    for (int e = 0; e < E; ++e) mm[e] = mask[(size_t)j * (E * 64) + e * 64 + lane];
    for (int i = 0; i < n; ++i) {
        load_col<E>(vecs[i], task, lane, xx);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double t = bcast(coef + (size_t)i * nreg, mm[e]) * xx[e];
            acc[e] = (i == 0) ? t : acc[e] + t;
        }
    }
    store_col<E>(out, task, lane, acc);
}

template <int E>
__global__ void k_mask(int ncol, int ny, double* __restrict__ v, const int32_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * NK2D_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (task >= ncol) return;
    const int j = task % ny;
    double vv[E];
    load_col<E>(v, task, lane, vv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int m = mask[(size_t)j * (E * 64) + e * 64 + lane];
        vv[e] = (m != 0) ? vv[e] : 0.0;
    }
    store_col<E>(v, task, lane, vv);
}

// region scalars (and vector pointers) of an algebra call: pageable caller memory -> pinned twin
// -> device.  Every entry point that stages coefficients synchronises before it returns, so the
// pinned twin is free again at the next call.
static int stage_coef(nk2d_ctx* c, const void* host, size_t n, size_t offset) {
    if (offset + n > c->rcoef_elems) return nk2d_fail(c, "region coefficient staging overflow");
    std::memcpy(c->hRCOEF + offset, host, sizeof(double) * n);
    NK2D_CHECK(c, hipMemcpyAsync(c->RCOEF + offset, c->hRCOEF + offset, sizeof(double) * n, hipMemcpyHostToDevice, nk2d_s(c)));
    return 0;
}

static int launch_dot(nk2d_ctx* c, const double* a, const double* b) {
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_dot<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c), c->ncol,
                                               c->ny, c->nreg, a, b, c->WN, c->MASK, c->PART));
    NK2D_CHECK(c, hipGetLastError());
    return 0;
}

extern "C" int nk2d_dot(nk2d_ctx* c, nk2d_vec a, nk2d_vec b, double* out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_TRY(launch_dot(c, (const double*)a, (const double*)b));
    return nk2d_k_reduce(c, c->ncol, c->nreg, out);
}

extern "C" int nk2d_axpby(nk2d_ctx* c, nk2d_vec out, const double* a, nk2d_vec x, const double* b, nk2d_vec y) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_TRY(stage_coef(c, a, c->nreg, 0));
    NK2D_TRY(stage_coef(c, b, c->nreg, c->nreg));
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_axpby<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c), c->ncol,
                                               c->ny, c->RCOEF, (const double*)x, c->RCOEF + c->nreg, (const double*)y,
                                               c->MASK, (double*)out));
    NK2D_CHECK(c, hipGetLastError());
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));  // RCOEF is reused by the next call
    return 0;
}

extern "C" int nk2d_scale(nk2d_ctx* c, nk2d_vec out, nk2d_vec x, const double* s) {
    return nk2d_diff_scale(c, out, x, nullptr, s);
}

extern "C" int nk2d_diff_scale(nk2d_ctx* c, nk2d_vec out, nk2d_vec x, nk2d_vec y, const double* s) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_TRY(stage_coef(c, s, c->nreg, 0));
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_diff_scale<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                               c->ncol, c->ny, (const double*)x, (const double*)y, c->RCOEF, c->MASK,
                                               (double*)out));
    NK2D_CHECK(c, hipGetLastError());
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}

extern "C" int nk2d_lin_comb(nk2d_ctx* c, nk2d_vec out, int32_t n, const nk2d_vec* vecs, const double* coef) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if (n < 1 || n > 512) return nk2d_fail(c, "nk2d_lin_comb: n out of range");
    // pointers are staged behind the coefficients (8-byte slots)
    const size_t ncoef = (size_t)n * c->nreg;
    if (ncoef + (size_t)n > c->rcoef_elems) return nk2d_fail(c, "nk2d_lin_comb: too many vectors");
    NK2D_TRY(stage_coef(c, coef, ncoef, 0));
    NK2D_TRY(stage_coef(c, vecs, (size_t)n, ncoef));  // pointers are 8-byte slots like the coefficients
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_lin_comb<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                               c->ncol, c->ny, n, c->nreg, (const double* const*)(c->RCOEF + ncoef),
                                               c->RCOEF, c->MASK, (double*)out));
    NK2D_CHECK(c, hipGetLastError());
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    return 0;
}

extern "C" int nk2d_mgs(nk2d_ctx* c, nk2d_vec w, int32_t n, const nk2d_vec* basis, double* h_out) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    if ((size_t)(n + 1) * c->nreg > 4096) return nk2d_fail(c, "nk2d_mgs: too many basis vectors");
    // sequential projections; each h_i stays on the device until the end
    for (int i = 0; i < n; ++i) {
        NK2D_TRY(launch_dot(c, (const double*)w, (const double*)basis[i]));
        // reduce into RED[(i+1)*nreg ...]; slot 0 is scratch of nk2d_k_reduce
        NK2D_TRY(nk2d_k_reduce(c, c->ncol, c->nreg, nullptr));
        NK2D_CHECK(c, hipMemcpyAsync(c->RED + (size_t)(i + 1) * c->nreg, c->RED, sizeof(double) * c->nreg,
                                     hipMemcpyDeviceToDevice, nk2d_s(c)));
        NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_mgs_update<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                                   c->ncol, c->ny, (double*)w, (const double*)basis[i],
                                                   c->RED + (size_t)(i + 1) * c->nreg, c->MASK));
        NK2D_CHECK(c, hipGetLastError());
    }
    if (n > 0) {
        NK2D_CHECK(c, hipMemcpyAsync(c->hRED, c->RED + c->nreg, sizeof(double) * n * c->nreg, hipMemcpyDeviceToHost, nk2d_s(c)));
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        std::memcpy(h_out, c->hRED, sizeof(double) * n * c->nreg);
    }
    return 0;
}

extern "C" int nk2d_apply_region_mask(nk2d_ctx* c, nk2d_vec v) {
    NK2D_CHECK(c, hipSetDevice(c->dev));
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_mask<EE>, dim3(nk2d_grid(c->ncol)), dim3(NK2D_BLOCK), 0, nk2d_s(c), c->ncol,
                                               c->ny, (double*)v, c->MASK));
    NK2D_CHECK(c, hipGetLastError());
    return 0;
}
