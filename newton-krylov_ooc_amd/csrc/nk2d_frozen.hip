// nk2d_frozen.hip -- the frozen year in ONE launch on a schedule cache (k_frozen_persistent).
#include "nk2d_bodies.h"

#include <algorithm>
#ifdef NK2D_FROZEN_CLOCKS
#include <cstdio>
#endif
#include <vector>

// the tables of row i of a cache in pieces: in the piece that holds the row
__device__ __forceinline__ RowTabs cache_row_tabs(const CachePiecePtrs& C, int i) {
    const int p = i / C.T.rows;
    return piece_row_tabs(C.C, C.T, C.T.base[p], i - p * C.T.rows);
}

// planes and Jacobian of every row: task = (row, slot 0..3, ypos column).  PIECES: the cache is a list of pieces (the planes'
// places are absolute addresses in the rows either way; the Jacobian's are resolved per row)
template <int E, int PIECES = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) k_cache_planes(DevP P, const CacheRow* __restrict__ rows, typename CacheArgOf<PIECES>::type C, int n) {
    const int lane = threadIdx.x & 63;
    const long long task = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long per_row = 4LL * P.ny;
    if (task >= per_row * n) return;
    const int i = (int)(task / per_row), rem = (int)(task - (long long)i * per_row);
    const int slot = rem / P.ny, j = rem - slot * P.ny;
    const CacheRow& R = rows[i];
    if (slot < 3) {
        double kv[E];
        vmix_body_kv<E>(P, R.v, slot * P.ny + j, lane, kv);
    } else {
        double kv[E], up[E], dn[E], so[E], no[E], ce[E];
        vmix_col_regs<E>(P, R.v.bldmin, R.v.y0, R.v.y1, R.v.hw, R.v.frac[3], j, lane, kv);
        jac_cols<E>(P, kv, j, lane, up, dn, so, no, ce);
        size_t np;
        double* J;
        if constexpr (PIECES) { np = C.C.np; J = cache_row_tabs(C, i).J; }
        else { np = C.np; J = C.J + (size_t)i * 5 * C.np; }
        store_col<E>(J, j, lane, up);
        store_col<E>(J + np, j, lane, dn);
        store_col<E>(J + 2 * np, j, lane, so);
        store_col<E>(J + 3 * np, j, lane, no);
        store_col<E>(J + 4 * np, j, lane, ce);
        if (R.v.out[3] != nullptr && P.f_sms > 0) {
            // a forced module with a thresholded sink (option "frozen_forced" bit 2): the file source at the row's Jacobian time,
            // vmix_body_kv's expressions with slot 3's records -- what the year forms UPR from
            double lo[E], hi[E], val[E];
            load_col<E>(P.SMSREC + (size_t)R.v.srec[3] * P.np, j, lane, lo);
            load_col<E>(P.SMSREC + (size_t)(R.v.srec[3] + 1) * P.np, j, lane, hi);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double slope = (hi[e] - lo[e]) / R.v.sden[3];
                val[e] = ((lane * E + e) < P.nz) ? slope * R.v.sdx[3] + lo[e] : 0.0;
            }
            store_col<E>(R.v.out[3], j, lane, val);
        }
    }
}

// line factorisation of every row: task = (row, (system, tracer), ypos column) -- the work of k_factor per row
template <int E, int KIND, int PIECES = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) k_cache_factor(DevP P, const CacheRow* __restrict__ rows, typename CacheArgOf<PIECES>::type C, int n) {
    const int lane = threadIdx.x & 63;
    const long long task = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long per_row = 2LL * P.ncol;
    if (task >= per_row * n) return;
    const int i = (int)(task / per_row), rem = (int)(task - (long long)i * per_row);
    const CacheRow& R = rows[i];
    SweepArgs A = {};
    if constexpr (PIECES) {
        const RowTabs t = cache_row_tabs(C, i);
        const size_t np = C.C.np;
        A.JL = t.J; A.JU = t.J + np; A.JS = t.J + 2 * np; A.JN = t.J + 3 * np; A.JC = t.J + 4 * np;
        A.fr_inv = t.fr_inv; A.fc_invr = t.fc_invr; A.fc_invi = t.fc_invi;
        A.fr_tab = t.fr_tab; A.fc_tabr = t.fc_tabr; A.fc_tabi = t.fc_tabi;
    } else {
        const double* J = C.J + (size_t)i * 5 * C.np;
        A.JL = J; A.JU = J + C.np; A.JS = J + 2 * C.np; A.JN = J + 3 * C.np; A.JC = J + 4 * C.np;
        A.fr_inv = C.fr_inv + (size_t)i * C.nv; A.fc_invr = C.fc_invr + (size_t)i * C.nv; A.fc_invi = C.fc_invi + (size_t)i * C.nv;
        A.fr_tab = C.fr_tab + (size_t)i * C.ntab; A.fc_tabr = C.fc_tabr + (size_t)i * C.ntab; A.fc_tabi = C.fc_tabi + (size_t)i * C.ntab;
    }
    A.f32 = 0;
    A.cre = R.cre; A.ccr = R.ccr; A.cci = R.cci;
    A.nreal = P.ncol; A.ntasks = 2 * P.ncol;
    factor_body<E, KIND>(P, A, rem, lane);
}

// The factorising first phase of a row of the LEAN one-launch year, a wave per column: newton_fused_body with FACTOR = 1.  Of
// what the year keeps in LDS it takes the coefficients and W (W lives nowhere else); the step block, a copy of what the cache
// row holds, it reads from memory like the command stream's factorising phase -- the same values.  Behind it the column's
// pivots of the real system, which it has just written, go to the wave's own LDS slot for the phases that follow (bit 8).
// (Three and more levels per lane; below that nothing of the year is in LDS and the phase is the plain factorising body.)
template <int E, int KIND, int MPX, int FINAL>
__device__ __forceinline__ void frozen_factor_phase(const DevP& P, const FusedArgs& FA, int wave, int lane, const FinalArgs* fin, const LdsSrc* L,
                                                    int coef_lds, bool w_in_lds, double* piv_lds) {
    if (w_in_lds) newton_fused_body<E, KIND, 1, 1, MPX, FINAL, 3>(P, FA, wave, lane, fin, L);
    else if (coef_lds) newton_fused_body<E, KIND, 1, 1, MPX, FINAL, 1>(P, FA, wave, lane, fin, L);
    else newton_fused_body<E, KIND, 1, 1, MPX, FINAL>(P, FA, wave, lane, fin);
    if (piv_lds) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the wave's own stores, read back by itself)
        double v[E];
        load_col<E>(FA.sw.fr_inv, wave, lane, v);
        w_lds_put<E>(piv_lds, 0, lane, v);
    }
}

// TEAM = 1: a workgroup is ONE column, its four waves the team of newton_team_body (a stage tendency each on three of them,
// the complex system on the fourth, exchanges through LDS): the phase of a small grid is the dependent arithmetic of one
// column's Newton iteration, and the team cuts that chain (three tendencies one after the other, then the real and the
// complex solve one after the other -> one tendency, then both solves side by side).  Same arithmetic, same bits.
// PIECES = 1: the cache is a list of pieces (option "frozen_cache_pieces", FrozenPieceArgs): once per row the piece's base comes
// from the device table by one scalar load and the row's eight table addresses are formed in scalar registers; the phases
// read them as the slab flavour reads its own.  Everything else is the one body.
// LEAN = 1: the cache holds the planes only (option "frozen_cache_lean"): the six factor-table pointers of A.C are ONE row's
// worth of tables, and the first phase of every row is the factorising instantiation of its body (FACTOR = 1, what the
// launch-per-phase path runs at every "LU" event) with the row's shifts: it leaves pivots and PCR tables of the wave's own
// column there, and the row's later phases -- the error estimate included -- read them as they read a full cache's.  A
// column's tables are written and read by its own workgroup only: nothing of them crosses the hand-over.
// The body of the kernel is the text of nk2d_frozen_body.inc, which its two entries include: k_frozen_persistent, and -- phosphorus
// from five levels per lane -- k_frozen_persistent_w2, the same within 256 registers (as k_stream has k_stream_w2).  Included text
// rather than a device function called by both: through a function the instantiations of k_frozen_persistent came out with
// other register counts (1 to 14 vector registers up or down on 38 of 80); as text they are what they were.
// A column's own state from phase to phase (OwnState, bits 16 and 32 of option "frozen_coef_lds"): the instantiations that carry it.
// A wave per column by column, the linear-source kinds, the full cache, five to seven levels per lane: the lean factorising
// phase and phosphorus keep their bodies, and at eight levels per lane neither the registers (421 of 512 before, one of them
// spilled) nor the LDS of a compute unit with two workgroups hold it (profiles/r09_frozen_own_state_resources.log)
#define NK2D_FROZEN_OWN(E, KIND, TEAM, LEAN) ((E) >= 5 && (E) <= 7 && ((KIND) == 0 || (KIND) == 2) && !(TEAM) && !(LEAN))
template <int E, int KIND, int TEAM = 0, int PIECES = 0, int LEAN = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) k_frozen_persistent(DevP P, typename FrozenArgOf<PIECES>::type A) {
#include "nk2d_frozen_body.inc"
}
// The same within 256 registers, so that a SIMD holds TWO waves (option "frozen_phosphorus" 2 and 3; phosphorus on the lean cache from
// five levels per lane, where a by-column workgroup of three waves at a wave per SIMD leaves the chip room for one workgroup per
// compute unit: 416 ypos columns are then two workgroups on each).  What does not fit the registers lives in scratch memory.
template <int E, int PIECES>
__global__ void __launch_bounds__(NK2D_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) k_frozen_persistent_w2(DevP P, typename FrozenArgOf<PIECES>::type A) {
    constexpr int KIND = 1, TEAM = 0, LEAN = 1;
#include "nk2d_frozen_body.inc"
}

// the cache of everything a schedule fixes besides the state; rebuilt when another schedule comes
struct nk2d_frozen_cache {
    uint64_t key = 0;
    int64_t n = 0;
    CachePtrs C = {};
    double* slab = nullptr;            // the one allocation the table pointers of C point into
    CacheRow* rows_dev = nullptr;      // [n]
    FrozenRow* frows_dev = nullptr;    // [n]
    size_t cap_rows = 0;
    std::vector<FrozenRow> frows;
    // a LARGE slab is allocated by a thread of its own (hipMalloc of 120 GB takes 0.03 - 3 s depending on what the process
    // holds on the host and the device): the years of the meantime run launch by launch
    std::thread alloc_thread;
    std::atomic<int> alloc_state{0};   // 0 nothing under way, 1 under way, 2 done (alloc_* valid), 3 failed
    double* alloc_slab = nullptr;
    CacheRow* alloc_rows = nullptr;
    FrozenRow* alloc_frows = nullptr;
    size_t alloc_cap = 0;
    // option "frozen_cache_pieces": the cache as a list of equally sized pieces instead of the slab -- never both.  Piece p
    // holds rows [p piece_rows, (p + 1) piece_rows), laid out inside as a slab of that many rows; pieces are kept from
    // schedule to schedule and only added to
    std::vector<double*> pieces;
    size_t piece_rows = 0;
    double** pieces_dev = nullptr;      // their bases on the device, [pieces_dev_cap]
    size_t pieces_dev_cap = 0;
    size_t rows_cap = 0;                // room of rows_dev / frows_dev in this form (they grow on their own)
    std::vector<double*> alloc_pieces;  // what the thread allocated (valid with alloc_state 2 and alloc_is_pieces)
    size_t alloc_piece_rows = 0;
    bool alloc_is_pieces = false;
    // option "frozen_cache_lean": the slab / the pieces hold the planes only (KV, J) -- never both forms at once -- and
    // `lean_tab` is the ONE row of factor tables (3 nv + 3 ntab doubles, allocated once) that the year's kernel fills row by row
    bool lean = false;
    bool alloc_lean = false;            // the form a thread's allocation was asked for
    double* lean_tab = nullptr;
    size_t lean_tab_doubles = 0;
    // option "frozen_forced" bit 2 (a forced module with a thresholded sink; lean only): every row also holds the file-source plane at
    // its Jacobian time (np doubles, behind J), and `upr` is the plane the year's kernel forms UPR in (nv doubles, allocated once):
    // the context's own UPR stays what the launch path left there
    bool src = false;
    bool alloc_src = false;
    double* upr = nullptr;
    size_t upr_doubles = 0;
};

// a forced module whose file source has a sink threshold: its Jacobian reads the state (the diagonal plane UPR)
static bool frozen_thres(const nk2d_ctx* c) { return c->kind == 2 && c->d.sms_nrec > 0 && c->d.sink_thres > 0.0; }

// phosphorus (module_kind 1) where option "frozen_phosphorus" lets it take the one-launch year: on the lean cache ("frozen_cache_lean" 1, or
// 2, which for such a context always means lean), at three to eight levels per lane -- the workgroup is then one ypos column with
// its tracers, a wave each.  One and two levels per lane stay out: the by-column workgroup does not exist there, and the
// four-wave teams cannot hold three coupled tracers
static bool frozen_phos(const nk2d_ctx* c) {
    return c->kind == 1 && c->frozen_phosphorus != 0 && c->frozen_cache_lean != 0 && c->E >= 3 && c->E <= 8 && c->tc <= NK2D_WAVES_PER_BLOCK;
}

// doubles of a row of the cache (lean: the planes only; src: and the file-source plane at the Jacobian time)
static size_t frozen_row_doubles(const nk2d_ctx* c, bool lean, bool src) {
    const size_t ntab = (size_t)c->ncol * NK2D_TAB * 64;
    return 3 * c->kv_len + 5 * c->np + (lean ? 0 : 3 * c->nv + 3 * ntab) + (src ? c->np : 0);
}

// rows per piece: option "frozen_cache_piece_rows", or what fits "frozen_cache_piece_mb" MiB (at least one)
static size_t frozen_piece_rows(const nk2d_ctx* c, bool lean, bool src) {
    if (c->frozen_cache_piece_rows > 0) return (size_t)c->frozen_cache_piece_rows;
    const double fit = std::floor(c->frozen_cache_piece_mb * 1048576.0 / (8.0 * (double)frozen_row_doubles(c, lean, src)));
    return fit >= 1.0 ? (size_t)std::min(fit, 1.0e9) : (size_t)1;
}

static void frozen_free_slab(nk2d_frozen_cache* fc) {
    if (fc->slab) (void)hipFree(fc->slab);
    if (fc->rows_dev) (void)hipFree(fc->rows_dev);
    if (fc->frows_dev) (void)hipFree(fc->frows_dev);
    fc->slab = nullptr; fc->rows_dev = nullptr; fc->frows_dev = nullptr; fc->cap_rows = 0;
    fc->C.KV = nullptr;
    fc->key = 0; fc->n = 0;
}

static void frozen_free_pieces(nk2d_frozen_cache* fc) {
    for (double* p : fc->pieces)
        if (p) (void)hipFree(p);
    fc->pieces.clear();
    fc->piece_rows = 0;
    if (fc->pieces_dev) (void)hipFree(fc->pieces_dev);
    fc->pieces_dev = nullptr; fc->pieces_dev_cap = 0;
    if (fc->rows_cap) {
        if (fc->rows_dev) (void)hipFree(fc->rows_dev);
        if (fc->frows_dev) (void)hipFree(fc->frows_dev);
        fc->rows_dev = nullptr; fc->frows_dev = nullptr; fc->rows_cap = 0;
    }
    fc->key = 0; fc->n = 0;
}

static uint64_t sched_key(const double* sched, int64_t n) {
    uint64_t h = 14695981039346656037ull;
    const unsigned char* p = (const unsigned char*)sched;
    const size_t nb = sizeof(double) * (size_t)n * NK2D_SCHED_WIDTH;
    for (size_t i = 0; i < nb; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h ? h : 1;
}

// what a schedule cache (and a command tape, option "frozen_tape") is kept for: the schedule, the context's fingerprint and the
// error-estimate stride
// (a LEAN cache of the same schedule has another key: a full cache is never read as a lean one; so has a lean cache with the
// file-source planes of option "frozen_forced" bit 2)
static const uint64_t FROZEN_LEAN_KEY = 0xC2B2AE3D27D4EB4Full;
static const uint64_t FROZEN_SRC_KEY = 0x165667B19E3779F9ull;
static const uint64_t FROZEN_PHOS_KEY = 0x27D4EB2F165667C5ull;      // (... and the lean cache of a phosphorus context, option "frozen_phosphorus")
uint64_t nk2d_frozen_key(const nk2d_ctx* c, const double* sched, int64_t n) {
    return sched_key(sched, n) ^ (uint64_t)nk2d_fingerprint(c) ^ ((uint64_t)(c->frozen_err_check + 1) * 0x9E3779B97F4A7C15ull);
}

// where the tables lie inside a piece: the slab's order, with room for piece_rows rows
static PieceTab frozen_piece_tab(const nk2d_ctx* c, const nk2d_frozen_cache* fc) {
    const size_t ntab = (size_t)c->ncol * NK2D_TAB * 64, B = fc->piece_rows;
    PieceTab T;
    T.base = fc->pieces_dev;
    T.rows = (int)B;
    T.oJ = B * 3 * c->kv_len;
    T.oS = 0;
    if (fc->lean) {     // (a piece ends behind J, or behind the source planes: the offsets of the absent tables are unused)
        T.ofr = T.ofcr = T.ofci = T.otr = T.otcr = T.otci = 0;
        if (fc->src) T.oS = T.oJ + B * 5 * c->np;
        return T;
    }
    T.ofr = T.oJ + B * 5 * c->np;
    T.ofcr = T.ofr + B * c->nv;
    T.ofci = T.ofcr + B * c->nv;
    T.otr = T.ofci + B * c->nv;
    T.otcr = T.otr + B * ntab;
    T.otci = T.otcr + B * ntab;
    return T;
}

// 1 while a thread is allocating the slab (or pieces) of this context's schedule cache
int nk2d_frozen_cache_pending(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    return (fc && fc->alloc_state.load() == 1) ? 1 : 0;
}

// bytes of HBM the schedule cache of this context holds right now
int64_t nk2d_frozen_cache_bytes(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) return 0;
    if (!fc->pieces.empty()) return (int64_t)(8 * fc->pieces.size() * fc->piece_rows * frozen_row_doubles(c, fc->lean, fc->src));
    if (!fc->slab) return 0;
    return (int64_t)(8 * fc->cap_rows * frozen_row_doubles(c, fc->lean, fc->src));
}

// 1 while the schedule cache this context holds is lean (option "frozen_cache_lean")
int nk2d_frozen_cache_is_lean(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    return (fc && fc->lean && (fc->slab || !fc->pieces.empty())) ? 1 : 0;
}

// pieces allocated for this context so far: those booked, and those a thread has finished allocating and the owner has not
// adopted yet (an allocation counts when it is made, not when the year that uses it comes)
int64_t nk2d_frozen_cache_piece_allocs(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    const bool waiting = fc && fc->alloc_state.load() == 2 && fc->alloc_is_pieces;
    return c->frozen_cache_piece_allocs + (waiting ? (int64_t)fc->alloc_pieces.size() : 0);
}

// pieces the schedule cache of this context holds right now (option "frozen_cache_pieces")
int64_t nk2d_frozen_cache_npieces(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    return fc ? (int64_t)fc->pieces.size() : 0;
}

void nk2d_frozen_cache_free(nk2d_ctx* c) {
    nk2d_frozen_cache* fc = (nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) return;
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    if (fc->alloc_state.load() == 2) {
        if (fc->alloc_slab) (void)hipFree(fc->alloc_slab);
        if (fc->alloc_rows) (void)hipFree(fc->alloc_rows);
        if (fc->alloc_frows) (void)hipFree(fc->alloc_frows);
        for (double* p : fc->alloc_pieces) (void)hipFree(p);
    }
    frozen_free_pieces(fc);
    frozen_free_slab(fc);
    if (fc->lean_tab) (void)hipFree(fc->lean_tab);
    if (fc->upr) (void)hipFree(fc->upr);
    delete fc;
    c->frozen_cache = nullptr;
}

// 0: the year ran in one launch (buffers in their roles after the last-but-one row's end; the last row's Newton iterations
//    done, its commit left to the caller);  1: not for this context / schedule (the launch-per-phase path runs);
// 2: a grid barrier timed out (the same);  < 0: error
// the instantiation for (levels per lane, module kind, flavour); the team flavour exists for one and two levels per lane
// `coop`: every workgroup of the grid must be resident at once (the grid-barrier and hand-over flavours: a workgroup waits
// for others).  Launched PLAINLY all the same: the launch is refused here (hipErrorCooperativeLaunchTooLarge) when the chip
// cannot hold the grid -- occupancy of the kernel times the compute units --, the process runs one resident kernel at a
// time (nk2d_turn_take), and every wait inside the kernel is bounded by time, so a grid that did not become fully
// resident after all (a co-tenant on the chip) hands the year back instead of hanging.  hipLaunchCooperativeKernel did the
// same check and nothing else for this kernel -- through a queue of its own that the HIP runtime crashed on when the process
// ended under rocprofv3 (rounds 2 - 3: AqlQueue::~AqlQueue under hsa_shut_down).
// doubles of dynamic shared memory of a wave-per-column workgroup of `nwaves` waves (the kernel's layout; bits: LdsSrc)
static size_t frozen_lds_doubles(int E, int bits, bool by_column, int nwaves) {
    if (!bits) return 0;
    if (!by_column) return (size_t)nwaves * (NK2D_COEF_LDS_DOUBLES(E) + ((bits & 2) ? 3 * E * 64 : 0));
    return NK2D_COEF_LDS_DOUBLES(E) + ((bits & 4) ? 5 * E * 64 : 0) +
           (size_t)nwaves * (((bits & 2) ? 3 * E * 64 : 0) + ((bits & 8) ? E * 64 : 0) + ((bits & 16) ? E * 64 : 0));
}

template <class K, class ARGS>
static hipError_t launch_resident(nk2d_ctx* c, K kernel, dim3 grid, dim3 block, DevP& P, ARGS& A, size_t lds_bytes = 0, bool check_only = false) {
    int per_cu = 0;
    hipError_t rc = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)block.x, lds_bytes);
    if (rc != hipSuccess) return rc;
    hipDeviceProp_t prop;
    rc = hipGetDeviceProperties(&prop, c->dev);
    if (rc != hipSuccess) return rc;
    if ((long long)per_cu * prop.multiProcessorCount < (long long)grid.x) return hipErrorCooperativeLaunchTooLarge;
    if (check_only) return hipSuccess;      // (the caller only asks whether the chip holds the grid)
    if (std::getenv("NK2D_DIAG_COOPERATIVE")) {
        // diagnostic only (profiles/r04_slowdown_ab.log): the launch as rounds 2 - 3 made it, through the runtime's cooperative queue
        void* args[2] = {&P, &A};
        return hipLaunchCooperativeKernel((const void*)kernel, grid, block, args, (unsigned)lds_bytes, nk2d_s(c));
    }
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, nk2d_s(c), P, A);
    return hipGetLastError();
}

template <int E, int KIND, int TEAM, int PIECES, int LEAN>
static hipError_t launch_frozen_one(nk2d_ctx* c, dim3 grid, DevP& P, typename FrozenArgOf<PIECES>::type& A) {
    // a team per column: the workgroup IS the column.  A wave per column: option "frozen_wpb" adjacent columns of one tracer to
    // a workgroup (its waves move in lock step, its neighbours are the workgroups to the left and right), or -- by_column --
    // one ypos column with all its tracers.  Three and more levels per lane: a wave's own data of the year in LDS
    const int wpb = TEAM ? NK2D_WAVES_PER_BLOCK : std::max(1, std::min(NK2D_WAVES_PER_BLOCK, c->frozen_wpb));
    const dim3 g = TEAM ? grid : dim3((unsigned)((c->ncol + wpb - 1) / wpb));
    if (!TEAM && E >= 3 && A.by_column)
        return launch_resident(c, k_frozen_persistent<E, KIND, TEAM, PIECES, LEAN>, dim3((unsigned)c->ny), dim3(64 * c->tc), P, A,
                               sizeof(double) * frozen_lds_doubles(E, A.coef_lds, true, c->tc));
    const size_t lds = (!TEAM && E >= 3 && A.coef_lds) ? sizeof(double) * frozen_lds_doubles(E, A.coef_lds, false, wpb) : 0;
    return launch_resident(c, k_frozen_persistent<E, KIND, TEAM, PIECES, LEAN>, g, dim3(64 * wpb), P, A, lds);
}
template <int KIND, int TEAM, int PIECES, int LEAN>
static hipError_t launch_frozen_e(nk2d_ctx* c, dim3 grid, DevP& P, typename FrozenArgOf<PIECES>::type& A) {
    switch (c->E) {
        case 1: return launch_frozen_one<1, KIND, TEAM, PIECES, LEAN>(c, grid, P, A);
        case 2: return launch_frozen_one<2, KIND, TEAM, PIECES, LEAN>(c, grid, P, A);
        // three and four levels per lane: a wave per column (all module kinds)
        case 3: if constexpr (!TEAM) return launch_frozen_one<3, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        case 4: if constexpr (!TEAM) return launch_frozen_one<4, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        // five to eight levels per lane (up to 512 levels): a wave per column; linear sources, and the file-driven forced module
        // (option "frozen_forced": frozen_eligible() lets it come here)
        case 5: if constexpr (!TEAM) return launch_frozen_one<5, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        case 6: if constexpr (!TEAM) return launch_frozen_one<6, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        case 7: if constexpr (!TEAM) return launch_frozen_one<7, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        case 8: if constexpr (!TEAM) return launch_frozen_one<8, KIND, 0, PIECES, LEAN>(c, grid, P, A); else break;
        default: break;
    }
    return hipErrorInvalidValue;
}
template <int PIECES, int LEAN>
static hipError_t launch_frozen(nk2d_ctx* c, bool team, dim3 grid, DevP& P, typename FrozenArgOf<PIECES>::type& A) {
    const bool forced = c->kind == 2;
    if (team) return forced ? launch_frozen_e<2, 1, PIECES, LEAN>(c, grid, P, A) : launch_frozen_e<0, 1, PIECES, LEAN>(c, grid, P, A);
    return forced ? launch_frozen_e<2, 0, PIECES, LEAN>(c, grid, P, A) : launch_frozen_e<0, 0, PIECES, LEAN>(c, grid, P, A);
}

// phosphorus (option "frozen_phosphorus"): always by column and lean; `two_waves`: the 256-register entry (five to eight levels per lane)
template <int E, int PIECES>
static hipError_t launch_frozen_phos_one(nk2d_ctx* c, DevP& P, typename FrozenArgOf<PIECES>::type& A, bool two_waves, bool check_only) {
    const dim3 grid((unsigned)c->ny), block((unsigned)(64 * c->tc));
    const size_t lds = sizeof(double) * frozen_lds_doubles(E, A.coef_lds, true, c->tc);
    if constexpr (E >= 5) {
        if (two_waves) return launch_resident(c, k_frozen_persistent_w2<E, PIECES>, grid, block, P, A, lds, check_only);
    } else if (two_waves) {
        return hipErrorInvalidValue;
    }
    return launch_resident(c, k_frozen_persistent<E, 1, 0, PIECES, 1>, grid, block, P, A, lds, check_only);
}
template <int PIECES>
static hipError_t launch_frozen_phos(nk2d_ctx* c, DevP& P, typename FrozenArgOf<PIECES>::type& A, bool two_waves, bool check_only = false) {
    if (!A.by_column || c->tc > NK2D_WAVES_PER_BLOCK) return hipErrorInvalidValue;
    switch (c->E) {
        case 3: return launch_frozen_phos_one<3, PIECES>(c, P, A, two_waves, check_only);
        case 4: return launch_frozen_phos_one<4, PIECES>(c, P, A, two_waves, check_only);
        case 5: return launch_frozen_phos_one<5, PIECES>(c, P, A, two_waves, check_only);
        case 6: return launch_frozen_phos_one<6, PIECES>(c, P, A, two_waves, check_only);
        case 7: return launch_frozen_phos_one<7, PIECES>(c, P, A, two_waves, check_only);
        case 8: return launch_frozen_phos_one<8, PIECES>(c, P, A, two_waves, check_only);
        default: break;
    }
    return hipErrorInvalidValue;
}

// the slab of a schedule cache with room for `cap` rows from a thread of the library's own (hipMalloc of 120 GB: 0.03 - 3 s);
// what the cache held before is given back by that thread first.  alloc_state 1 while it runs, 2 / 3 when done / refused
static void frozen_alloc_in_thread(nk2d_frozen_cache* fc, int dev, size_t slab_bytes, size_t cap, double* old_slab, CacheRow* old_rows,
                                   FrozenRow* old_frows, bool lean, bool src) {
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    fc->alloc_state.store(1);
    fc->alloc_is_pieces = false;
    fc->alloc_lean = lean;
    fc->alloc_src = src;
    fc->alloc_thread = std::thread([fc, dev, slab_bytes, cap, old_slab, old_rows, old_frows]() {
        bool ok = hipSetDevice(dev) == hipSuccess;
        if (old_slab) (void)hipFree(old_slab);
        if (old_rows) (void)hipFree(old_rows);
        if (old_frows) (void)hipFree(old_frows);
        fc->alloc_slab = nullptr; fc->alloc_rows = nullptr; fc->alloc_frows = nullptr;
        ok = ok && hipMalloc((void**)&fc->alloc_slab, slab_bytes) == hipSuccess;
        ok = ok && hipMalloc((void**)&fc->alloc_rows, sizeof(CacheRow) * cap) == hipSuccess;
        ok = ok && hipMalloc((void**)&fc->alloc_frows, sizeof(FrozenRow) * cap) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (fc->alloc_slab) (void)hipFree(fc->alloc_slab);
            if (fc->alloc_rows) (void)hipFree(fc->alloc_rows);
            if (fc->alloc_frows) (void)hipFree(fc->alloc_frows);
        }
        fc->alloc_cap = cap;
        fc->alloc_state.store(ok ? 2 : 3);
    });
}

// `count` more pieces of `piece_bytes` each from that thread (a cache in pieces): all of them or none -- on a refused piece
// this request's pieces are given back and the state is 3.  The owner adopts them when the state says 2, none before
static void frozen_alloc_pieces_in_thread(nk2d_frozen_cache* fc, int dev, size_t piece_bytes, size_t count, size_t piece_rows, bool lean, bool src) {
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    fc->alloc_state.store(1);
    fc->alloc_is_pieces = true;
    fc->alloc_lean = lean;
    fc->alloc_src = src;
    fc->alloc_piece_rows = piece_rows;
    fc->alloc_pieces.clear();
    fc->alloc_thread = std::thread([fc, dev, piece_bytes, count]() {
        bool ok = hipSetDevice(dev) == hipSuccess;
        for (size_t k = 0; ok && k < count; ++k) {
            double* p = nullptr;
            ok = hipMalloc((void**)&p, piece_bytes) == hipSuccess;
            if (ok) fc->alloc_pieces.push_back(p);
        }
        if (!ok) {
            (void)hipGetLastError();
            for (double* p : fc->alloc_pieces) (void)hipFree(p);
            fc->alloc_pieces.clear();
        }
        fc->alloc_state.store(ok ? 2 : 3);
    });
}

// what a thread was asked for: 1 not there yet, 3 refused, 0 nothing under way (any more: what it allocated is the cache's now)
static int frozen_adopt(nk2d_ctx* c, nk2d_frozen_cache* fc) {
    const int st = fc ? fc->alloc_state.load() : 0;
    if (st == 0 || st == 1) return st;
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    fc->alloc_state.store(0);
    if (st == 3) return 3;
    if (fc->alloc_is_pieces) {
        // (asked for with the rows per piece of the pieces held, if any: none is freed or added while a request is under way)
        c->frozen_cache_piece_allocs += (int64_t)fc->alloc_pieces.size();
        fc->pieces.insert(fc->pieces.end(), fc->alloc_pieces.begin(), fc->alloc_pieces.end());
        fc->piece_rows = fc->alloc_piece_rows;
        fc->lean = fc->alloc_lean;      // (pieces held before the request were of the same form: the other form goes first)
        fc->src = fc->alloc_src;
        fc->alloc_pieces.clear();
        return 0;
    }
    fc->lean = fc->alloc_lean;
    fc->src = fc->alloc_src;
    fc->slab = fc->alloc_slab; fc->rows_dev = fc->alloc_rows; fc->frows_dev = fc->alloc_frows; fc->cap_rows = fc->alloc_cap;
    fc->alloc_slab = nullptr; fc->alloc_rows = nullptr; fc->alloc_frows = nullptr;
    fc->C.KV = nullptr;     // (the tables' places are set at the build)
    return 0;
}

// is the one-launch year made for this context and schedule?
static bool frozen_eligible(const nk2d_ctx* c, const double* sched, int64_t n) {
    // a Jacobian that reads the state: a forced module with a thresholded sink with option "frozen_forced" bit 2, phosphorus with
    // option "frozen_phosphorus" -- both on the lean cache only (their full cache -- factorisations ahead of the state -- cannot exist)
    const bool thres = frozen_thres(c);
    const bool phos = frozen_phos(c);
    const bool needs_state = (c->kind == 1 && !phos) || (thres && !((c->frozen_forced & 2) && c->frozen_cache_lean != 0));
    if (!c->frozen_persistent || needs_state || c->hist_n != 0 || c->norm_hook || n < 1) return false;
    // the cache holds the factorisation in double precision only: with option "factor_fp32" the recorded year read the single
    // precision copies, and the one-launch year would not be the same discrete map (round-3 ADVICE) -- launch by launch then
    if (c->factor_fp32) return false;
    // (one to four levels per lane; five to eight with linear sources -- for the file-driven forced module there with option
    // "frozen_forced": bit 1 without, bit 2 with a sink threshold)
    if (c->E > c->frozen_persistent_max_e || c->E > 8) return false;
    if (c->E > 4 && c->kind != 0 && !phos && !(c->kind == 2 && (c->frozen_forced & (thres ? 2 : 1)))) return false;
    if (thres || phos) {
        // UPR is formed where the launch path evaluates the Jacobian anew (replay_rows): at a step start, or -- option
        // "jac_stage_state" -- at a stage time of the row's own attempt.  A schedule it would refuse goes to it, to be refused
        const double RCs[3] = {0.15505102572168222, 0.6449489742783178, 1.0};
        double t_jac_prev = c->d.t0;
        for (int64_t i = 0; i < n; ++i) {
            const double* r = sched + i * NK2D_SCHED_WIDTH;
            const double t = r[0], h = r[2], t_jac = r[4];
            if (t_jac != t_jac_prev && t_jac != t) {
                bool at_stage = false;
                for (int k = 0; k < 3 && c->jac_stage_state; ++k) at_stage = at_stage || t_jac == t + (h * RCs[k]);
                if (!at_stage) return false;
            }
            t_jac_prev = t_jac;
        }
    }
    // every row but the last must hand over to the next one (t_new == next t, whole step taken): the step-ending launch
    // predicts the next attempt from this step's collocation polynomial
    for (int64_t i = 0; i + 1 < n; ++i) {
        const double* r = sched + i * NK2D_SCHED_WIDTH;
        if (!(r[0] + r[2] == r[1] && r[NK2D_SCHED_WIDTH] == r[1] && r[NK2D_SCHED_WIDTH + 2] > 0.0 && (int)r[3] >= 1)) return false;
    }
    return (int)sched[(n - 1) * NK2D_SCHED_WIDTH + 3] >= 1;
}

// The form of the cache of a schedule of `n` rows (option "frozen_cache_lean"; key_full: its key as a full cache).  0: full, 1: lean,
// 2: lean only where the full cache would be refused -- by "frozen_cache_gb", or by the 85 % rule where it would have to be
// allocated.  What a thread is allocating stays what it is, and so does a lean cache the 85 % rule chose for this very schedule
// (the device is not asked again every year); "frozen_cache_gb" is looked at every time.
static int frozen_form(nk2d_ctx* c, int64_t n, uint64_t key_full, bool* lean) {
    *lean = c->frozen_cache_lean == 1;
    if (frozen_thres(c) || c->kind == 1) { *lean = true; return 0; }    // (eligible with a lean cache only: "frozen_cache_lean" 2 always means lean here)
    if (c->frozen_cache_lean != 2) return 0;
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    if (fc && fc->alloc_state.load() != 0) { *lean = fc->alloc_lean; return 0; }
    const bool holds = fc && (fc->slab || !fc->pieces.empty());
    const bool pieces = c->frozen_cache_pieces != 0;
    const size_t B = pieces ? frozen_piece_rows(c, false, false) : 1, rows = ((size_t)n + B - 1) / B * B;
    const double bytes = 8.0 * (double)rows * (double)frozen_row_doubles(c, false, false);
    if (bytes > c->frozen_cache_max_gb * 1.0e9) { *lean = true; return 0; }
    if (holds && !fc->lean) {       // (room enough in the full form already: nothing to allocate, nothing to refuse)
        if (pieces ? (fc->piece_rows == B && fc->pieces.size() * B >= rows) : (fc->slab && fc->cap_rows >= (size_t)n)) return 0;
    }
    if (holds && fc->lean && fc->n == n && fc->key == (key_full ^ FROZEN_LEAN_KEY) && c->frozen_lean_mem_key == key_full) { *lean = true; return 0; }
    size_t free_b = 0, total_b = 0;
    NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
    *lean = 1.02 * bytes > 0.85 * ((double)free_b + (double)nk2d_frozen_cache_bytes(c));
    c->frozen_lean_mem_key = *lean ? key_full : 0;
    return 0;
}

// Options "frozen_cache_pieces" + "frozen_cache_early": the pieces for the `n` rows of the schedule a free-running year just
// recorded are asked for NOW, from the thread whatever their size, so that they are there when the first product comes; the
// tables are built where they always are, at the first frozen year.  (With the slab this was measured and taken out, see
// below; pieces are what makes the request one the driver can serve beside other allocations -- or not: DESIGN 3.6.)
int nk2d_frozen_cache_early(nk2d_ctx* c, const double* sched, int64_t n) {
    if (!c->frozen_cache_pieces || !c->frozen_cache_early || !sched || !frozen_eligible(c, sched, n)) return 0;
    bool want_lean = false;
    NK2D_TRY(frozen_form(c, n, nk2d_frozen_key(c, sched, n), &want_lean));
    const bool want_src = frozen_thres(c);
    const size_t per_row = frozen_row_doubles(c, want_lean, want_src), B = frozen_piece_rows(c, want_lean, want_src), need = ((size_t)n + B - 1) / B;
    const double bytes = 8.0 * (double)need * (double)B * (double)per_row;
    if (bytes > c->frozen_cache_max_gb * 1.0e9) return 0;
    nk2d_frozen_cache* fc = (nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) { fc = new nk2d_frozen_cache(); c->frozen_cache = fc; }
    const int st = frozen_adopt(c, fc);
    if (st == 1) return 0;
    if (st == 3) { c->frozen_persistent = 0; return 0; }
    if (fc->slab || (!fc->pieces.empty() && (fc->piece_rows != B || fc->lean != want_lean || fc->src != want_src))) {
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        frozen_free_slab(fc);
        frozen_free_pieces(fc);
    }
    if (fc->pieces.size() >= need) return 0;
    size_t free_b = 0, total_b = 0;
    NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
    const double held = 8.0 * (double)fc->pieces.size() * (double)B * (double)per_row;
    if (1.02 * bytes > 0.85 * ((double)free_b + held)) return 0;
    frozen_alloc_pieces_in_thread(fc, c->dev, sizeof(double) * B * per_row, need - fc->pieces.size(), B, want_lean, want_src);
    c->frozen_cache_early_requests++;
    return 0;
}

// what lives in LDS (option "frozen_coef_lds", bits of LdsSrc) and which columns share a workgroup (option "frozen_by_column"):
// as much as lets a compute unit hold what the grid needs of it -- ceil(waves / compute units) waves: pivots, then the step
// block, then W are given up until it fits the 160 KB (E = 8 keeps everything but the pivots).  The column's own state (bits 16:
// Y in LDS, given up before anything else, and 32: the stage values in registers) exists in the instantiations
// NK2D_FROZEN_OWN names, by column, on top of everything else: with a part of 15 missing both bits go; a cache in pieces has
// the stage values only together with Y
static int frozen_lds_shape(nk2d_ctx* c, bool phos, bool lean, bool pieces, int* coef_lds_out, int* by_column_out) {
    int coef_lds = (c->E >= 3) ? c->frozen_coef_lds : 0;
    // (by column -- and with it the step block and the pivots -- from five levels per lane: 416^2 125.2 -> 120.3 ms; at four the shared
    // block does not pay for the wider hand-over, 208^2 65.2 -> 68.1 ms: profiles/r04_frozen_lds_by_column.log; option value 2 forces it)
    int by_column = (c->frozen_by_column && c->tc <= NK2D_WAVES_PER_BLOCK && coef_lds &&
                     (c->E >= 5 || (c->frozen_by_column >= 2 && c->E >= 3))) ? 1 : 0;
    // (phosphorus: its tracers are coupled inside a ypos column -- by column whatever the two options say, "frozen_coef_lds" 0 included)
    if (phos) by_column = 1;
    if (!by_column) coef_lds &= 3;
    const bool team = c->frozen_team && c->E <= 2;
    if (!by_column || phos || (coef_lds & 15) != 15 || !NK2D_FROZEN_OWN(c->E, c->kind, team, lean)) coef_lds &= 15;
    hipDeviceProp_t prop;
    NK2D_CHECK(c, hipGetDeviceProperties(&prop, c->dev));
    const int nw = by_column ? c->tc : std::max(1, std::min(NK2D_WAVES_PER_BLOCK, c->frozen_wpb));
    const int wgs = by_column ? c->ny : (c->ncol + nw - 1) / nw;
    const int per_cu = (wgs + prop.multiProcessorCount - 1) / prop.multiProcessorCount;
    for (const int drop : {16, 8, 4, 2}) {
        if (8 * frozen_lds_doubles(c->E, coef_lds, by_column != 0, nw) * (size_t)per_cu <= 160u * 1024u) break;
        coef_lds &= ~drop;
    }
    if ((coef_lds & 15) != 15) coef_lds &= 15;
    if (pieces && (coef_lds & 48) == 32) coef_lds &= 15;      // (the piece flavour has no body for the stage values without Y)
    *coef_lds_out = coef_lds; *by_column_out = by_column;
    return 0;
}

// (Asking for that slab EARLIER -- at the end of the free-running year whose steps the products will repeat, so that it is
// there when the first product comes -- was built and measured in round 4 and taken out again: in a fresh process the
// hipMalloc of 120 GB holds the driver for ~ 4 s, and the preconditioner's set-up, which lies between F(x) and the first
// product and allocates its 10 GB of inverses, waited behind it: set-up 0.50 -> 4.18 s, spin-up of iage 416 x 416 3.98 / 5.14 ->
// 9.34 s (profiles/r04_prealloc_experiment.log).  Beside the first products, which allocate nothing, the same request costs
// them 0.1 - 1.2 s in all.)
int nk2d_frozen_persistent(nk2d_ctx* c, const double* sched, int64_t n, std::vector<char>* err_rows) {
    if (!frozen_eligible(c, sched, n)) return 1;
    const size_t ntab = (size_t)c->ncol * NK2D_TAB * 64;
    // the cache as pieces (option "frozen_cache_pieces"): `need` pieces of `B` rows; the limits apply to their sum
    const bool want_pieces = c->frozen_cache_pieces != 0;
    // lean (option "frozen_cache_lean"): rows of planes only; the limits apply to that size.  Its key is another
    const uint64_t key_full = nk2d_frozen_key(c, sched, n);
    bool want_lean = false;
    NK2D_TRY(frozen_form(c, n, key_full, &want_lean));
    // (a thresholded forced module -- eligible with option "frozen_forced" bit 2 only, and lean: a row holds its source plane too)
    const bool want_src = frozen_thres(c);
    // (phosphorus -- eligible with option "frozen_phosphorus" only, and lean: a row is KV and J, the light plane is the context's own)
    const bool want_phos = c->kind == 1;
    const size_t per_row = frozen_row_doubles(c, want_lean, want_src);
    const size_t B = want_pieces ? frozen_piece_rows(c, want_lean, want_src) : 0, need = want_pieces ? ((size_t)n + B - 1) / B : 0;
    const double bytes = want_pieces ? 8.0 * (double)need * (double)B * (double)per_row : 8.0 * (double)n * (double)per_row;
    if (bytes > c->frozen_cache_max_gb * 1.0e9) return 1;
    if (want_phos) {
        // whether the chip holds the grid is known before anything is allocated or built (416 ypos columns at one wave per SIMD are
        // the expected case that it does not): the occupancy check of the launch, asked ahead, for the flavours the option's value allows
        FrozenPieceArgs A0 = {};
        NK2D_TRY(frozen_lds_shape(c, true, true, want_pieces, &A0.coef_lds, &A0.by_column));
        DevP P0 = make_devp(c);
        const bool has_w2 = c->E >= 5;
        auto fits = [&](bool w2) {
            return want_pieces ? launch_frozen_phos<1>(c, P0, A0, w2, true) : launch_frozen_phos<0>(c, P0, static_cast<FrozenArgs&>(A0), w2, true);
        };
        hipError_t rc = fits(has_w2 && c->frozen_phosphorus == 3);
        if (rc == hipErrorCooperativeLaunchTooLarge && has_w2 && c->frozen_phosphorus == 2) rc = fits(true);
        if (rc == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return 1; }
        NK2D_CHECK(c, rc);
    }
    {   // what a thread was asked for: not there yet (launch by launch), there (adopt it), or refused (never again)
        const int st = frozen_adopt(c, (nk2d_frozen_cache*)c->frozen_cache);
        if (st == 1) return 1;
        if (st == 3) { c->frozen_persistent = 0; return 1; }
    }
    if (nk2d_frozen_cache* have = (nk2d_frozen_cache*)c->frozen_cache) {
        // a context never holds a slab and pieces at once, nor a full and a lean cache: the other form (and pieces of another
        // size) go first
        const bool other_form = have->lean != want_lean || have->src != want_src;
        const bool drop_slab = have->slab && (want_pieces || other_form);
        const bool drop_pieces = !have->pieces.empty() && (!want_pieces || have->piece_rows != B || other_form);
        if (drop_slab || drop_pieces) {
            NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
            if (drop_slab) frozen_free_slab(have);
            if (drop_pieces) frozen_free_pieces(have);
        }
    }
    {   // ... and never more than what the device has to spare right now (other contexts of the process, other tenants)
        nk2d_frozen_cache* have = (nk2d_frozen_cache*)c->frozen_cache;
        if (want_pieces) {
            const size_t held_n = have ? have->pieces.size() : 0;
            if (held_n < need) {
                size_t free_b = 0, total_b = 0;
                NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
                const double held = 8.0 * (double)held_n * (double)B * (double)per_row;
                if (1.02 * bytes > 0.85 * ((double)free_b + held)) return 1;
            }
        } else if (!have || have->cap_rows < (size_t)n) {
            size_t free_b = 0, total_b = 0;
            NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
            const double held = have ? 8.0 * (double)have->cap_rows * (double)per_row : 0.0;
            if (1.02 * bytes > 0.85 * ((double)free_b + held)) return 1;
        }
    }
    nk2d_frozen_cache* fc = (nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) { fc = new nk2d_frozen_cache(); c->frozen_cache = fc; }
    // (the rows also say which steps carry an error estimate)
    const uint64_t key = key_full ^ (want_lean ? FROZEN_LEAN_KEY : 0) ^ (want_src ? FROZEN_SRC_KEY : 0) ^ (want_phos ? FROZEN_PHOS_KEY : 0);
    if (fc->key != key || fc->n != n) {
        // option "frozen_cache_after": that many years of a schedule run launch by launch before its cache is built.  Default
        // 0; -1: 0 for caches below 8 GB, 3 above.  Building a 100 GB cache takes 26 ms where a one-launch year saves 40
        // (tools/probe_cache_build.py) -- but its FIRST allocation has been seen to take 0.8 s inside a Newton run, and a Newton
        // iteration with two or three Krylov iterations has nothing to pay that back with; a long Krylov solve has.
        const int after = c->frozen_cache_after >= 0 ? c->frozen_cache_after : (bytes > 8.0e9 ? 3 : 0);
        if (c->frozen_seen_key != key) { c->frozen_seen_key = key; c->frozen_seen_years = 0; }
        if (c->frozen_seen_years++ < after) return 1;
    }
    DevP P = make_devp(c);
    if (fc->key != key || fc->n != n) {
        // ---- (re)build the cache for this schedule
        if (want_lean && fc->lean_tab_doubles < 3 * c->nv + 3 * ntab) {
            // the one row of factor tables the lean year's kernel works in: allocated once
            NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
            if (fc->lean_tab) (void)hipFree(fc->lean_tab);
            fc->lean_tab = nullptr; fc->lean_tab_doubles = 0;
            NK2D_CHECK(c, hipMalloc((void**)&fc->lean_tab, sizeof(double) * (3 * c->nv + 3 * ntab)));
            fc->lean_tab_doubles = 3 * c->nv + 3 * ntab;
        }
        if ((want_src || want_phos) && fc->upr_doubles < (want_phos ? c->np : c->nv)) {
            // the plane the year's kernel forms UPR in: allocated once (phosphorus: one plane, d uptake / d po4)
            const size_t upr_doubles = want_phos ? c->np : c->nv;
            NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
            if (fc->upr) (void)hipFree(fc->upr);
            fc->upr = nullptr; fc->upr_doubles = 0;
            NK2D_CHECK(c, hipMalloc((void**)&fc->upr, sizeof(double) * upr_doubles));
            fc->upr_doubles = upr_doubles;
        }
        if (want_pieces) {
            if (fc->pieces.size() < need) {
                // more pieces, no headroom rows: what is there stays where it is
                NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
                const size_t add = need - fc->pieces.size(), piece_bytes = sizeof(double) * B * per_row;
                fc->key = 0; fc->n = 0;
                if ((double)add * (double)piece_bytes > 8.0e9 && c->frozen_alloc_async) {
                    // (piece by piece from the thread: launch by launch until all of them are there)
                    frozen_alloc_pieces_in_thread(fc, c->dev, piece_bytes, add, B, want_lean, want_src);
                    return 1;
                }
                const size_t before = fc->pieces.size();
                for (size_t k = 0; k < add; ++k) {
                    double* p = nullptr;
                    const hipError_t rc = hipMalloc((void**)&p, piece_bytes);
                    if (rc != hipSuccess) {     // (this request's pieces are given back)
                        for (size_t q = before; q < fc->pieces.size(); ++q) (void)hipFree(fc->pieces[q]);
                        fc->pieces.resize(before);
                        NK2D_CHECK(c, rc);
                    }
                    fc->pieces.push_back(p);
                }
                fc->piece_rows = B;
                fc->lean = want_lean;
                fc->src = want_src;
                c->frozen_cache_piece_allocs += (int64_t)add;
            }
            if (fc->rows_cap < (size_t)n) {
                NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
                if (fc->rows_dev) (void)hipFree(fc->rows_dev);
                if (fc->frows_dev) (void)hipFree(fc->frows_dev);
                fc->rows_dev = nullptr; fc->frows_dev = nullptr; fc->rows_cap = 0;
                NK2D_CHECK(c, hipMalloc((void**)&fc->rows_dev, sizeof(CacheRow) * (size_t)n));
                NK2D_CHECK(c, hipMalloc((void**)&fc->frows_dev, sizeof(FrozenRow) * (size_t)n));
                fc->rows_cap = (size_t)n;
            }
            if (fc->pieces_dev_cap < fc->pieces.size()) {
                NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
                if (fc->pieces_dev) (void)hipFree(fc->pieces_dev);
                fc->pieces_dev = nullptr; fc->pieces_dev_cap = 0;
                NK2D_CHECK(c, hipMalloc((void**)&fc->pieces_dev, sizeof(double*) * fc->pieces.size()));
                fc->pieces_dev_cap = fc->pieces.size();
            }
            NK2D_CHECK(c, hipMemcpy(fc->pieces_dev, fc->pieces.data(), sizeof(double*) * fc->pieces.size(), hipMemcpyHostToDevice));
            fc->C.KV = fc->C.J = fc->C.fr_inv = fc->C.fc_invr = fc->C.fc_invi = fc->C.fr_tab = fc->C.fc_tabr = fc->C.fc_tabi = nullptr;
        } else if (fc->cap_rows < (size_t)n) {
            // ONE allocation for the whole cache, with room for the longer schedules of later Newton iterates: giving 100 GB
            // back and asking for them again costs seconds (measured inside a Newton run: 4.4 s), the first request 0.03 - 0.8 s
            NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
            // (what this cache holds now is given back first -- by the thread, where a thread allocates)
            double* old_slab = fc->slab;
            CacheRow* old_rows = fc->rows_dev;
            FrozenRow* old_frows = fc->frows_dev;
            const double held_b = 8.0 * (double)fc->cap_rows * (double)per_row;
            fc->slab = nullptr; fc->rows_dev = nullptr; fc->frows_dev = nullptr; fc->cap_rows = 0;
            fc->key = 0; fc->n = 0;
            size_t cap = (size_t)n + (size_t)n / 6 + 16;
            {
                size_t free_b = 0, total_b = 0;
                NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
                const size_t fit = (size_t)(0.9 * ((double)free_b + held_b) / (8.0 * (double)per_row));
                cap = std::max((size_t)n, std::min(cap, fit));
            }
            const size_t slab_bytes = sizeof(double) * cap * per_row;
            const bool in_thread = slab_bytes > (size_t)8e9 && c->frozen_alloc_async;
            if (!in_thread) {
                if (old_slab) (void)hipFree(old_slab);
                if (old_rows) (void)hipFree(old_rows);
                if (old_frows) (void)hipFree(old_frows);
            }
            if (in_thread) {
                // (the new slab and tables come from the thread: launch by launch until they are there)
                frozen_alloc_in_thread(fc, c->dev, slab_bytes, cap, old_slab, old_rows, old_frows, want_lean, want_src);
                return 1;
            }
            NK2D_CHECK(c, hipMalloc((void**)&fc->slab, slab_bytes));
            NK2D_CHECK(c, hipMalloc((void**)&fc->rows_dev, sizeof(CacheRow) * cap));
            NK2D_CHECK(c, hipMalloc((void**)&fc->frows_dev, sizeof(FrozenRow) * cap));
            fc->cap_rows = cap;
            fc->lean = want_lean;
            fc->src = want_src;
        }
        if (!want_pieces && want_lean) {
            fc->C.KV = fc->slab;
            fc->C.J = fc->slab + fc->cap_rows * 3 * c->kv_len;
        } else if (!want_pieces && (fc->C.KV != fc->slab || fc->C.nv != c->nv || fc->C.fr_inv == fc->lean_tab)) {   // (a new slab: the tables' places in it)
            const size_t cap = fc->cap_rows;
            double* p = fc->slab;
            fc->C.KV = p; p += cap * 3 * c->kv_len;
            fc->C.J = p; p += cap * 5 * c->np;
            fc->C.fr_inv = p; p += cap * c->nv;
            fc->C.fc_invr = p; p += cap * c->nv;
            fc->C.fc_invi = p; p += cap * c->nv;
            fc->C.fr_tab = p; p += cap * ntab;
            fc->C.fc_tabr = p; p += cap * ntab;
            fc->C.fc_tabi = p;
        }
        if (want_lean) {    // (slab or pieces: the six factor tables are the one row)
            double* p = fc->lean_tab;
            fc->C.fr_inv = p; p += c->nv;
            fc->C.fc_invr = p; p += c->nv;
            fc->C.fc_invi = p; p += c->nv;
            fc->C.fr_tab = p; p += ntab;
            fc->C.fc_tabr = p; p += ntab;
            fc->C.fc_tabi = p;
        }
        fc->C.kv_len = c->kv_len; fc->C.np = c->np; fc->C.nv = c->nv; fc->C.ntab = ntab;
        const double RCs[3] = {0.15505102572168222, 0.6449489742783178, 1.0};
        const double MU_REAL = 3.637834252744496, MU_CR = 2.6810828736277523, MU_CI = -3.050430199247411;
        std::vector<CacheRow> rows((size_t)n);
        fc->frows.assign((size_t)n, FrozenRow());
        for (int64_t i = 0; i < n; ++i) {
            const double* r = sched + i * NK2D_SCHED_WIDTH;
            const double t = r[0], t_new = r[1], h = r[2], t_jac = r[4], h_lu = r[5];
            CacheRow& R = rows[(size_t)i];
            double times[4];
            for (int k = 0; k < 3; ++k) times[k] = t + (h * RCs[k]);
            times[3] = t_jac;
            for (int k = 0; k < 4; ++k) {
                nk2d_host_interp(4, c->d.bld_tvals, c->d.bld_fvals, times[k], &R.v.frac[k]);
                if (want_pieces) R.v.out[k] = (k < 3) ? fc->pieces[(size_t)i / B] + (((size_t)i % B) * 3 + k) * c->kv_len : nullptr;
                else R.v.out[k] = (k < 3) ? fc->C.KV + ((size_t)i * 3 + k) * c->kv_len : nullptr;
            }
            // (slot 3 of a thresholded forced module: where the file source at the Jacobian time goes, behind the J planes)
            if (want_src) R.v.out[3] = want_pieces ? fc->pieces[(size_t)i / B] + B * (3 * c->kv_len + 5 * c->np) + ((size_t)i % B) * c->np
                                                   : fc->C.J + fc->cap_rows * 5 * c->np + (size_t)i * c->np;
            vmix_forcing_args(c, want_src ? 4 : 3, times, R.v);
            R.v.bldmin = c->d.bldepth_min; R.v.y0 = c->d.vmix_log_shallow; R.v.y1 = c->d.vmix_log_deep; R.v.hw = c->d.vmix_half_width;
            R.cre = MU_REAL / h_lu; R.ccr = MU_CR / h_lu; R.cci = MU_CI / h_lu;
            FrozenRow& F = fc->frows[(size_t)i];
            F.mreal = MU_REAL / h; F.mcr = MU_CR / h; F.mci = MU_CI / h;
            F.n_iter = (int)r[3];
            int m_real = nk2d_sweeps_for(c, MU_REAL / h_lu), m_cplx = nk2d_sweeps_for(c, MU_CR / h_lu);
            if (c->min_sweeps > 1 && nk2d_has_lateral(c)) { m_real = std::max(m_real, 2); m_cplx = std::max(m_cplx, 2); }
            F.m = std::max(m_real, m_cplx);
            F.h = h;
            F.cre = R.cre; F.ccr = R.ccr; F.cci = R.cci;
            // (single-sweep solves only: the estimate is then the column's own; two-sweep rows go unsampled)
            F.err = (c->frozen_err_check > 0 && i > 0 && i + 1 < n && (i % c->frozen_err_check) == 0 && F.m == 1 && F.n_iter >= 1) ? 1 : 0;
            // (the launch path evaluates the Jacobian where t_jac changes -- replay_rows; the year's first row: from the state it starts at)
            F.upr = (i == 0 || t_jac != sched[(i - 1) * NK2D_SCHED_WIDTH + 4]) ? 1 : 0;
            F.x0 = F.x1 = F.x2 = 1.0;
            if (i + 1 < n) {
                const double h2 = r[NK2D_SCHED_WIDTH + 2];
                F.x0 = ((t_new + h2 * RCs[0]) - t) / (t_new - t);
                F.x1 = ((t_new + h2 * RCs[1]) - t) / (t_new - t);
                F.x2 = ((t_new + h2 * RCs[2]) - t) / (t_new - t);
            }
        }
        NK2D_CHECK(c, hipMemcpyAsync(fc->rows_dev, rows.data(), sizeof(CacheRow) * (size_t)n, hipMemcpyHostToDevice, nk2d_s(c)));
        NK2D_CHECK(c, hipMemcpyAsync(fc->frows_dev, fc->frows.data(), sizeof(FrozenRow) * (size_t)n, hipMemcpyHostToDevice, nk2d_s(c)));
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));    // `rows` leaves scope
        if (want_pieces) {
            CachePiecePtrs CP;
            CP.C = fc->C;
            CP.T = frozen_piece_tab(c, fc);
            const long long tasks = 4LL * c->ny * n;
            NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL((k_cache_planes<EE, 1>), dim3((unsigned)((tasks + 3) / 4)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                                      P, fc->rows_dev, CP, (int)n));
            NK2D_CHECK(c, hipGetLastError());
            c->st.nlaunch += 1;
            if (!want_lean) {
                const long long ftasks = 2LL * c->ncol * n;
                NK2D_DISPATCH_EK(c->E, c->kind, hipLaunchKernelGGL((k_cache_factor<EE, KK, 1>), dim3((unsigned)((ftasks + 3) / 4)), dim3(NK2D_BLOCK), 0,
                                                                   nk2d_s(c), P, fc->rows_dev, CP, (int)n));
                NK2D_CHECK(c, hipGetLastError());
                c->st.nlaunch += 1;
            }
        } else {
            const long long tasks = 4LL * c->ny * n;
            NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL(k_cache_planes<EE>, dim3((unsigned)((tasks + 3) / 4)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                                      P, fc->rows_dev, fc->C, (int)n));
            NK2D_CHECK(c, hipGetLastError());
            c->st.nlaunch += 1;
            if (!want_lean) {
                const long long ftasks = 2LL * c->ncol * n;
                NK2D_DISPATCH_EK(c->E, c->kind, hipLaunchKernelGGL((k_cache_factor<EE, KK>), dim3((unsigned)((ftasks + 3) / 4)), dim3(NK2D_BLOCK), 0,
                                                                   nk2d_s(c), P, fc->rows_dev, fc->C, (int)n));
                NK2D_CHECK(c, hipGetLastError());
                c->st.nlaunch += 1;
            }
        }
        fc->key = key;
        fc->n = n;
        c->frozen_cache_builds++;
    }
    // a cache in pieces: every piece that covers rows < n must be there -- the kernel never looks at a missing one
    if (want_pieces) {
        if (fc->piece_rows != B || fc->lean != want_lean || fc->src != want_src || fc->pieces.size() < need || !fc->pieces_dev || fc->pieces_dev_cap < need) return 1;
        for (size_t p = 0; p < need; ++p)
            if (!fc->pieces[p]) return 1;
    }
    // ---- the year
    if (!c->YR_OUT) {
        NK2D_CHECK(c, hipMalloc((void**)&c->YR_PART, sizeof(double) * 2 * c->ncol));
        NK2D_CHECK(c, hipMalloc((void**)&c->YR_OUT, sizeof(double) * 32));
        NK2D_CHECK(c, hipMalloc((void**)&c->YR_SYNC, yr_sync_bytes(c)));
        NK2D_CHECK(c, hipMalloc((void**)&c->YR_MTAB, sizeof(int) * std::max<size_t>(c->rho_tab.size(), 1)));
        NK2D_CHECK(c, hipHostMalloc((void**)&c->hYR_OUT, sizeof(double) * 32));
        NK2D_CHECK(c, hipEventCreate(&c->yr_ev[0]));
        NK2D_CHECK(c, hipEventCreate(&c->yr_ev[1]));
        c->yr_lin_tol = -1.0;
        c->yr_rec_cap = 0;
        c->YR_REC = nullptr;
    }
    NK2D_CHECK(c, hipMemsetAsync(c->YR_SYNC, 0, yr_sync_bytes(c), nk2d_s(c)));
    FrozenPieceArgs A = {};      // (the slab flavour takes its FrozenArgs part)
    if (want_pieces) A.T = frozen_piece_tab(c, fc);
    A.Y = c->Y; A.YOLD = c->YOLD; A.Z = c->Z; A.ZN = c->ZN; A.W = c->W; A.F = c->F;
    A.BR = c->BR; A.BCR = c->BCR; A.BCI = c->BCI;
    for (int i = 0; i < 2; ++i) { A.XR[i] = c->XR[i]; A.XCR[i] = c->XCR[i]; A.XCI[i] = c->XCI[i]; }
    A.PART = c->YR_PART;
    A.STEP_PART = c->STEP_PART;
    A.rows = fc->frows_dev;
    A.C = fc->C;
    A.n = (int)n;
    A.arrive = (unsigned*)c->YR_SYNC; A.abort_flag = (int*)((char*)c->YR_SYNC + 4096);
    A.out = c->YR_OUT;
    A.spin_ticks = (long long)(c->barrier_timeout_ms * 1.0e5);
    A.fences = c->year_fences;
    // a thresholded forced module: the year forms UPR, in the cache's own plane, from the rows' source planes
    // (phosphorus: from the state and the context's light plane alone.  A year that is handed back leaves the context's own UPR what the
    // launch path left there)
    A.upr_on = (want_src || want_phos) ? 1 : 0;
    A.SRC = (want_src && !want_pieces) ? fc->C.J + fc->cap_rows * 5 * c->np : nullptr;
    if (want_src || want_phos) P.UPR = fc->upr;
    NK2D_TRY(frozen_lds_shape(c, want_phos, want_lean, want_pieces, &A.coef_lds, &A.by_column));
    c->frozen_lds_bits = A.coef_lds;
    c->frozen_early_bits = (A.coef_lds & 48) == 48 ? c->frozen_early : 0;   // (48 is there only where the own state is compiled in: frozen_lds_shape)
    // (invariant: bit 8 only together with bits 0 - 5.  Everything that takes A.coef_lds from here on -- frozen_lds_doubles() in the
    // launch functions, the kernel -- tests bits below 64 or non-zero, which bit 8 on top of 63 does not change)
    A.coef_lds |= c->frozen_early_bits << 8;
    // option "frozen_team": a workgroup per column (four waves: newton_team_body) instead of a wave per column, up to two levels per
    // lane.  Measured in round 3 (profiles/r03_frozen_team.log, r03_frozen_nbsync.log): teams want a CU each and beat the
    // wave-per-column year at every such size -- 26^2 9.4 ms, 52^2 14.9, 104^2 27.0 with the neighbour hand-over.
    const bool team = c->frozen_team && c->E <= 2;
    const int nblk = team ? c->ncol : nk2d_grid(c->ncol);
    const double* o = c->hYR_OUT;
    {
        A.spin_ticks = (long long)(c->barrier_timeout_ms * 1.0e5);
        hipError_t rc = hipErrorInvalidValue;
        NK2D_CHECK(c, hipMemsetAsync(c->YR_OUT, 0, sizeof(double) * 32, nk2d_s(c)));
        NK2D_CHECK(c, hipEventRecord(c->yr_ev[0], nk2d_s(c)));
        // one resident kernel at a time in this process (the turn is held until this one has ended)
        struct Turn {
            int waves;
            explicit Turn(int w) : waves(w) { nk2d_turn_take(waves); }
            ~Turn() { nk2d_turn_give(waves); }
        } turn(team ? 4 * c->ncol : c->ncol);
        c->frozen_two_waves_last = 0;
        if (want_phos) {
            // option "frozen_phosphorus": 1 the flavour of one wave per SIMD, where the chip holds its grid; 2 where it does not, the
            // 256-register flavour, if the chip holds that one; 3 the 256-register flavour wherever it exists (five to eight levels per lane)
            const bool has_w2 = c->E >= 5;
            bool two = has_w2 && c->frozen_phosphorus == 3;
            auto go = [&](bool w2) {
                return want_pieces ? launch_frozen_phos<1>(c, P, A, w2) : launch_frozen_phos<0>(c, P, static_cast<FrozenArgs&>(A), w2);
            };
            rc = go(two);
            if (rc == hipErrorCooperativeLaunchTooLarge && !two && has_w2 && c->frozen_phosphorus == 2) {
                (void)hipGetLastError();
                two = true;
                rc = go(two);
            }
            c->frozen_two_waves_last = two ? 1 : 0;
        }
        else if (want_lean) rc = want_pieces ? launch_frozen<1, 1>(c, team, dim3(nblk), P, A) : launch_frozen<0, 1>(c, team, dim3(nblk), P, static_cast<FrozenArgs&>(A));
        else rc = want_pieces ? launch_frozen<1, 0>(c, team, dim3(nblk), P, A) : launch_frozen<0, 0>(c, team, dim3(nblk), P, static_cast<FrozenArgs&>(A));
        if (rc == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return 1; }
        NK2D_CHECK(c, rc);
        NK2D_CHECK(c, hipEventRecord(c->yr_ev[1], nk2d_s(c)));
        NK2D_CHECK(c, hipMemcpyAsync(c->hYR_OUT, c->YR_OUT, sizeof(double) * 32, hipMemcpyDeviceToHost, nk2d_s(c)));
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        if ((int)o[0] != 0 || (int64_t)o[1] != n) return 2;
#ifdef NK2D_FROZEN_CLOCKS
        std::fprintf(stderr, "frozen clocks (early %d): %.0f phases, per phase drain %.3f us, flag store to poll match %.3f us, rest %.3f us; kernel %.3f ms\n",
                     c->frozen_early_bits, o[11], 0.01 * o[8] / o[11], 0.01 * o[9] / o[11], 0.01 * (o[10] - o[8] - o[9]) / o[11], 1.0e-5 * o[10]);
#endif
    }
    if (team) c->frozen_team_years++;
    {   // the launch itself, between two events on the context's stream (bench.py's roofline of the one-launch year)
        float ms = 0.f;
        NK2D_CHECK(c, hipEventElapsedTime(&ms, c->yr_ev[0], c->yr_ev[1]));
        c->frozen_launch_us += (int64_t)(1000.0 * (double)ms);
    }
    if ((int)o[2]) std::swap(c->Y, c->YOLD);
    if ((int)o[3]) std::swap(c->Z, c->ZN);
    // counters of the year, as the launch-per-phase path books them, and the algorithmic bytes of its phases (the formula of
    // the launches they replace; nothing of the schedule cache's one-off construction)
    for (int64_t i = 0; i < n; ++i) {
        const FrozenRow& F = fc->frows[(size_t)i];
        c->st.nnewton += F.n_iter; c->st.nfev += 3 * (int64_t)F.n_iter; c->st.nsolve += 2 * (int64_t)F.n_iter;
        c->st.nsweeps += (int64_t)F.n_iter * F.m;
        double words = 0.0;
        for (int it = 0; it < F.m; ++it) words += fused_words(c, it == 0, it == 0, it == F.m - 1, F.m == 2, false);
        c->fused_bytes_all += 8.0 * words * F.n_iter;
    }
    if (err_rows) {
        err_rows->assign((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i)
            if (fc->frows[(size_t)i].err) { (*err_rows)[(size_t)i] = 1; c->st.nerr_checked++; c->st.nfev++; c->st.nsolve++; }
    }
    c->sweep_launches += 1;
    c->st.nsteps += n - 1;      // the last row's commit is the caller's
    c->st.njev += n; c->st.nlu += 2 * n;
    c->st.nlaunch += 1;
    return 0;
}

