// nk2d_frozen.hip -- the frozen year in ONE launch on a schedule cache (k_frozen_persistent).
#include "nk2d_bodies.h"
#include "nk2d_frozen_plan.h"

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
// A column's own state from phase to phase (OwnState, bits 16 and 32 of option "frozen_coef_lds"): the instantiations that carry it are
// those NK2D_FROZEN_OWN names (nk2d_frozen_plan.h: the macro the planner fits the LDS with).
template <int E, int KIND, int TEAM = 0, int PIECES = 0, int LEAN = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) k_frozen_persistent(DevP P, typename FrozenArgOf<PIECES>::type A) {
#define FZ_ONLY 0
#include "nk2d_frozen_body.inc"
#undef FZ_ONLY
}
// The same within 256 registers, so that a SIMD holds TWO waves (option "frozen_phosphorus" 2 and 3; phosphorus on the lean cache from
// five levels per lane, where a by-column workgroup of three waves at a wave per SIMD leaves the chip room for one workgroup per
// compute unit: 416 ypos columns are then two workgroups on each).  What does not fit the registers lives in scratch memory.
template <int E, int PIECES>
__global__ void __launch_bounds__(NK2D_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) k_frozen_persistent_w2(DevP P, typename FrozenArgOf<PIECES>::type A) {
    constexpr int KIND = 1, TEAM = 0, LEAN = 1;
#define FZ_ONLY 0
#include "nk2d_frozen_body.inc"
#undef FZ_ONLY
}

// ---- the store: everything a schedule fixes besides the state, kept for the schedule `key`; rebuilt when another schedule comes.
// Its arithmetic -- forms, sizes, limits, growth, where a row's tables lie -- is nk2d_frozen_plan.h's.
struct nk2d_frozen_cache {
    uint64_t key = 0;
    int64_t n = 0;
    // the storage, in ONE form at a time: `blocks` of `block_rows` rows each, every block laid out by frozen_layout().  The slab
    // (pieces == false) is one block with head-room; with option "frozen_cache_pieces" block p holds rows [p block_rows,
    // (p + 1) block_rows), and blocks are kept from schedule to schedule and only added to.  lean (option "frozen_cache_lean"): the
    // blocks hold the planes only (KV, J); src (option "frozen_forced" bit 2, lean only): and every row's file-source plane
    std::vector<double*> blocks;
    size_t block_rows = 0;
    bool pieces = false, lean = false, src = false;
    double** blocks_dev = nullptr;      // the bases of pieces on the device, [blocks_dev_cap]
    size_t blocks_dev_cap = 0;
    CacheRow* rows_dev = nullptr;       // [rows_cap]
    FrozenRow* frows_dev = nullptr;     // [rows_cap]
    size_t rows_cap = 0;
    std::vector<FrozenRow> frows;
    // allocated once: `lean_tab`, the ONE row of factor tables (3 nv + 3 ntab doubles) that the lean year's kernel fills row by
    // row, and `upr`, the plane the year's kernel forms UPR in (src: nv doubles, phosphorus: np) -- the context's own UPR stays
    // what the launch path left there
    double* lean_tab = nullptr;
    size_t lean_tab_doubles = 0;
    double* upr = nullptr;
    size_t upr_doubles = 0;
    // blocks asked for from a thread of the library's own (frozen_growth(): why): alloc_state 0 nothing under way, 1 under way,
    // 2 done (`got` valid), 3 refused; `asked_*`: the request
    std::thread alloc_thread;
    std::atomic<int> alloc_state{0};
    FrozenPlan asked_form = {};
    FrozenGrowth asked = {};
    std::vector<double*> got;
};

static FrozenPlanIn frozen_plan_in(const nk2d_ctx* c) {
    FrozenPlanIn in = {};
    in.E = c->E; in.kind = c->kind; in.tc = c->tc; in.ny = c->ny; in.ncol = c->ncol;
    in.np = c->np; in.nv = c->nv; in.kv_len = c->kv_len;
    in.sms_nrec = c->d.sms_nrec; in.sink_thres = c->d.sink_thres; in.t0 = c->d.t0;
    in.frozen_persistent = c->frozen_persistent; in.frozen_persistent_max_e = c->frozen_persistent_max_e;
    in.frozen_forced = c->frozen_forced; in.frozen_phosphorus = c->frozen_phosphorus;
    in.frozen_phosphorus_shallow = c->frozen_phosphorus_shallow;
    in.frozen_cache_lean = c->frozen_cache_lean; in.frozen_cache_pieces = c->frozen_cache_pieces;
    in.frozen_cache_piece_mb = c->frozen_cache_piece_mb; in.frozen_cache_piece_rows = c->frozen_cache_piece_rows;
    in.frozen_cache_max_gb = c->frozen_cache_max_gb; in.frozen_cache_after = c->frozen_cache_after;
    in.frozen_alloc_async = c->frozen_alloc_async; in.frozen_err_check = c->frozen_err_check;
    in.frozen_coef_lds = c->frozen_coef_lds; in.frozen_by_column = c->frozen_by_column; in.frozen_wpb = c->frozen_wpb;
    in.frozen_team = c->frozen_team; in.factor_fp32 = c->factor_fp32; in.jac_stage_state = c->jac_stage_state;
    in.hist_n = c->hist_n; in.norm_hook = c->norm_hook != nullptr;
    return in;
}

static FrozenHeld frozen_held(const nk2d_ctx* c) {
    FrozenHeld h;
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) return h;
    h.pieces = fc->pieces; h.lean = fc->lean; h.src = fc->src;
    h.blocks = fc->blocks.size(); h.block_rows = fc->block_rows;
    h.alloc_state = fc->alloc_state.load(); h.alloc_lean = fc->asked_form.lean;
    h.key = fc->key; h.n = fc->n;
    return h;
}

static nk2d_frozen_cache* frozen_store(nk2d_ctx* c) {
    if (!c->frozen_cache) c->frozen_cache = new nk2d_frozen_cache();
    return (nk2d_frozen_cache*)c->frozen_cache;
}

uint64_t nk2d_frozen_key(const nk2d_ctx* c, const double* sched, int64_t n) {
    return frozen_key_full(frozen_plan_in(c), frozen_sched_hash(sched, n), (uint64_t)nk2d_fingerprint(c));
}

// 1 while a thread is allocating blocks of this context's schedule cache
int nk2d_frozen_cache_pending(const nk2d_ctx* c) { return frozen_held(c).alloc_state == 1 ? 1 : 0; }

// bytes of HBM the schedule cache of this context holds right now
int64_t nk2d_frozen_cache_bytes(const nk2d_ctx* c) { return (int64_t)frozen_held_bytes(frozen_plan_in(c), frozen_held(c)); }

// 1 while the schedule cache this context holds is lean (option "frozen_cache_lean")
int nk2d_frozen_cache_is_lean(const nk2d_ctx* c) {
    const FrozenHeld h = frozen_held(c);
    return (h.lean && h.blocks) ? 1 : 0;
}

// pieces allocated for this context so far: those booked, and those a thread has finished allocating and the owner has not
// adopted yet (an allocation counts when it is made, not when the year that uses it comes)
int64_t nk2d_frozen_cache_piece_allocs(const nk2d_ctx* c) {
    const nk2d_frozen_cache* fc = (const nk2d_frozen_cache*)c->frozen_cache;
    const bool waiting = fc && fc->alloc_state.load() == 2 && fc->asked_form.pieces;
    return c->frozen_cache_piece_allocs + (waiting ? (int64_t)fc->got.size() : 0);
}

// pieces the schedule cache of this context holds right now (option "frozen_cache_pieces")
int64_t nk2d_frozen_cache_npieces(const nk2d_ctx* c) {
    const FrozenHeld h = frozen_held(c);
    return h.pieces ? (int64_t)h.blocks : 0;
}

// the blocks and what goes with them are given back: the store holds nothing (lean_tab and upr stay)
static void frozen_free_blocks(nk2d_frozen_cache* fc) {
    for (double* p : fc->blocks)
        if (p) (void)hipFree(p);
    fc->blocks.clear();
    fc->block_rows = 0;
    if (fc->blocks_dev) (void)hipFree(fc->blocks_dev);
    if (fc->rows_dev) (void)hipFree(fc->rows_dev);
    if (fc->frows_dev) (void)hipFree(fc->frows_dev);
    fc->blocks_dev = nullptr; fc->blocks_dev_cap = 0;
    fc->rows_dev = nullptr; fc->frows_dev = nullptr; fc->rows_cap = 0;
    fc->key = 0; fc->n = 0;
}

void nk2d_frozen_cache_free(nk2d_ctx* c) {
    nk2d_frozen_cache* fc = (nk2d_frozen_cache*)c->frozen_cache;
    if (!fc) return;
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    if (fc->alloc_state.load() == 2)
        for (double* p : fc->got) (void)hipFree(p);
    frozen_free_blocks(fc);
    if (fc->lean_tab) (void)hipFree(fc->lean_tab);
    if (fc->upr) (void)hipFree(fc->upr);
    delete fc;
    c->frozen_cache = nullptr;
}

// `count` blocks of `bytes` each: all of them or none -- on a refused one this request's blocks are given back
static hipError_t frozen_alloc_blocks(size_t count, size_t bytes, std::vector<double*>* got) {
    got->clear();
    for (size_t k = 0; k < count; ++k) {
        double* p = nullptr;
        const hipError_t rc = hipMalloc((void**)&p, bytes);
        if (rc != hipSuccess) {
            for (double* q : *got) (void)hipFree(q);
            got->clear();
            return rc;
        }
        got->push_back(p);
    }
    return hipSuccess;
}

// blocks that were asked for in the form `pl` are the store's now (blocks held before are of the same form and size: the
// other form goes first, and none is freed or added while a request is under way)
static void frozen_take_blocks(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenPlan& pl, const FrozenGrowth& g, std::vector<double*>* got) {
    fc->blocks.insert(fc->blocks.end(), got->begin(), got->end());
    fc->block_rows = g.block_rows;
    fc->pieces = pl.pieces; fc->lean = pl.lean; fc->src = pl.src;
    if (pl.pieces) c->frozen_cache_piece_allocs += (int64_t)got->size();
    got->clear();
}

// the blocks of `g` from a thread of the library's own; `give_back` is given back by that thread first.  alloc_state 1 while it
// runs, 2 / 3 when done / refused: the owner adopts them when the state says 2, none before
static void frozen_request(nk2d_frozen_cache* fc, int dev, const FrozenPlan& pl, const FrozenGrowth& g, std::vector<double*> give_back) {
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    fc->alloc_state.store(1);
    fc->asked_form = pl;
    fc->asked = g;
    fc->alloc_thread = std::thread([fc, dev, g, give_back]() {
        bool ok = hipSetDevice(dev) == hipSuccess;
        for (double* p : give_back) (void)hipFree(p);
        ok = ok && frozen_alloc_blocks(g.count, g.block_bytes, &fc->got) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        fc->alloc_state.store(ok ? 2 : 3);
    });
}

// what a thread was asked for: 1 not there yet, 3 refused, 0 nothing under way (any more: what it allocated is the store's now)
static int frozen_adopt(nk2d_ctx* c, nk2d_frozen_cache* fc) {
    const int st = fc->alloc_state.load();
    if (st == 0 || st == 1) return st;
    if (fc->alloc_thread.joinable()) fc->alloc_thread.join();
    fc->alloc_state.store(0);
    if (st == 3) return 3;
    frozen_take_blocks(c, fc, fc->asked_form, fc->asked, &fc->got);
    return 0;
}

// ---- the launch: the instantiation for (levels per lane, module kind, flavour); the team flavour exists for one and two levels
// per lane.  Every workgroup of the grid must be resident at once (the grid-barrier and hand-over flavours: a workgroup waits
// for others).  Launched PLAINLY all the same: the launch is refused here (hipErrorCooperativeLaunchTooLarge) when the chip
// cannot hold the grid -- occupancy of the kernel times the compute units --, the process runs one resident kernel at a
// time (nk2d_turn_take), and every wait inside the kernel is bounded by time, so a grid that did not become fully
// resident after all (a co-tenant on the chip) hands the year back instead of hanging.  hipLaunchCooperativeKernel did the
// same check and nothing else for this kernel -- through a queue of its own that the HIP runtime crashed on when the process
// ended under rocprofv3 (rounds 2 - 3: AqlQueue::~AqlQueue under hsa_shut_down).

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

// the same for k_frozen_persistent_d, which lives in a unit of its own (nk2d_frozen_d.hip): always by column, everything in LDS
static hipError_t launch_resident_dedicated(nk2d_ctx* c, bool pieces, DevP& P, FrozenPieceArgs& A) {
    if (!A.by_column || c->tc > NK2D_WAVES_PER_BLOCK) return hipErrorInvalidValue;
    const dim3 grid((unsigned)c->ny), block((unsigned)(64 * c->tc));
    const size_t lds_bytes = sizeof(double) * frozen_lds_doubles(c->E, A.coef_lds, true, c->tc);
    int per_cu = 0;
    hipError_t rc = nk2d_frozen_launch_d(c, grid, block, P, A, pieces, &per_cu, lds_bytes);
    if (rc != hipSuccess) return rc;
    hipDeviceProp_t prop;
    rc = hipGetDeviceProperties(&prop, c->dev);
    if (rc != hipSuccess) return rc;
    if ((long long)per_cu * prop.multiProcessorCount < (long long)grid.x) return hipErrorCooperativeLaunchTooLarge;
    return nk2d_frozen_launch_d(c, grid, block, P, A, pieces, nullptr, lds_bytes);
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

// phosphorus (option "frozen_phosphorus"): always by column and lean; `two_waves`: the 256-register entry (five to eight levels per lane).
// Below three levels per lane frozen_lds_doubles() is 0: no dynamic LDS
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
        // one and two levels per lane (option "frozen_phosphorus_shallow"): nothing of the year in LDS, the one-wave flavour only
        case 1: return launch_frozen_phos_one<1, PIECES>(c, P, A, two_waves, check_only);
        case 2: return launch_frozen_phos_one<2, PIECES>(c, P, A, two_waves, check_only);
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

// phosphorus, option "frozen_phosphorus": 1 the flavour of one wave per SIMD, where the chip holds its grid; 2 where it does not, the
// 256-register flavour, if the chip holds that one; 3 the 256-register flavour wherever it exists (five to eight levels per lane).
// check_only: nothing is launched, the answer is whether the chip holds the grid of a flavour the option's value allows
static hipError_t launch_frozen_phos_flavour(nk2d_ctx* c, bool pieces, DevP& P, FrozenPieceArgs& A, bool check_only, bool* two_waves) {
    const bool has_w2 = c->E >= 5;
    auto go = [&](bool w2) {
        return pieces ? launch_frozen_phos<1>(c, P, A, w2, check_only) : launch_frozen_phos<0>(c, P, static_cast<FrozenArgs&>(A), w2, check_only);
    };
    *two_waves = has_w2 && c->frozen_phosphorus == 3;
    hipError_t rc = go(*two_waves);
    if (rc == hipErrorCooperativeLaunchTooLarge && !*two_waves && has_w2 && c->frozen_phosphorus == 2) {
        (void)hipGetLastError();
        *two_waves = true;
        rc = go(true);
    }
    return rc;
}

// ---- the steps of a one-launch year, in the order nk2d_frozen_persistent() takes them.  A step returns 0 to go on, 1 to hand the
// year to the launch-per-phase path, < 0 on an error

// plan: the form (the device is asked only where the 85 % rule has to decide), the sizes, the key
static int frozen_make_plan(nk2d_ctx* c, const FrozenPlanIn& in, const double* sched, int64_t n, FrozenPlan* pl) {
    const uint64_t key_full = nk2d_frozen_key(c, sched, n);
    const FrozenHeld held = frozen_held(c);
    bool ruled = false;
    int lean = frozen_form(in, n, key_full, held, c->frozen_lean_mem_key, nullptr, &ruled);
    if (lean < 0) {
        size_t free_b = 0, total_b = 0;
        NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
        const double free_bytes = (double)free_b;
        lean = frozen_form(in, n, key_full, held, c->frozen_lean_mem_key, &free_bytes, &ruled);
    }
    if (ruled) c->frozen_lean_mem_key = lean ? key_full : 0;
    *pl = frozen_plan(in, n, key_full, lean == 1);
    return pl->allowed ? 0 : 1;
}

static int frozen_fit_lds(nk2d_ctx* c, const FrozenPlanIn& in, const FrozenPlan& pl, int* coef_lds, int* by_column) {
    hipDeviceProp_t prop;
    NK2D_CHECK(c, hipGetDeviceProperties(&prop, c->dev));
    frozen_lds_shape(in, pl.phos, pl.lean, pl.pieces, prop.multiProcessorCount, coef_lds, by_column);
    return 0;
}

// phosphorus: whether the chip holds the grid is known before anything is allocated or built (416 ypos columns at one wave per SIMD
// are the expected case that it does not): the occupancy check of the launch, asked ahead
static int frozen_phos_resident(nk2d_ctx* c, const FrozenPlanIn& in, const FrozenPlan& pl) {
    FrozenPieceArgs A0 = {};
    NK2D_TRY(frozen_fit_lds(c, in, pl, &A0.coef_lds, &A0.by_column));
    DevP P0 = make_devp(c);
    bool two = false;
    const hipError_t rc = launch_frozen_phos_flavour(c, pl.pieces, P0, A0, true, &two);
    if (rc == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return 1; }
    NK2D_CHECK(c, rc);
    return 0;
}

// what a thread was asked for: not there yet (launch by launch), there (the store's now), or refused (never again)
static int frozen_thread_done(nk2d_ctx* c, nk2d_frozen_cache* fc) {
    const int st = frozen_adopt(c, fc);
    if (st == 3) c->frozen_persistent = 0;
    return st == 0 ? 0 : 1;
}

static int frozen_drop_other_form(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenPlan& pl) {
    if (!frozen_other_form(pl, frozen_held(c))) return 0;
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    frozen_free_blocks(fc);
    return 0;
}

// admission (frozen_admit), asked only where storage has to be allocated
static int frozen_admitted(nk2d_ctx* c, const FrozenPlanIn& in, const FrozenPlan& pl, int64_t n) {
    const FrozenHeld held = frozen_held(c);
    if (!frozen_must_grow(pl, held, n)) return 0;
    size_t free_b = 0, total_b = 0;
    NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));
    return frozen_admit(pl.bytes, (double)free_b, frozen_held_bytes(in, held)) ? 0 : 1;
}

// option "frozen_cache_after": 1 while the schedule's first years still run launch by launch
static int frozen_deferred(nk2d_ctx* c, const FrozenPlanIn& in, const FrozenPlan& pl) {
    if (c->frozen_seen_key != pl.key) { c->frozen_seen_key = pl.key; c->frozen_seen_years = 0; }
    return c->frozen_seen_years++ < frozen_years_before_build(in, pl.bytes) ? 1 : 0;
}

// a device array that grows on its own: at least `want` elements of `elem` bytes (what it held is not kept)
static int frozen_grow(nk2d_ctx* c, void** p, size_t* cap, size_t want, size_t elem) {
    if (*cap >= want) return 0;
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    NK2D_CHECK(c, hipMalloc(p, elem * want));
    *cap = want;
    return 0;
}

// the blocks for the n rows (frozen_growth(): inline, or 1 -- asked from the thread: launch by launch until they are there)
static int frozen_ensure_blocks(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenPlanIn& in, const FrozenPlan& pl, int64_t n) {
    const FrozenHeld held = frozen_held(c);
    if (!frozen_must_grow(pl, held, n)) return 0;
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    size_t free_b = 0, total_b = 0;
    if (!pl.pieces) NK2D_CHECK(c, hipMemGetInfo(&free_b, &total_b));     // (the slab's head-room is what the device has room for)
    const FrozenGrowth g = frozen_growth(in, pl, held, n, (double)free_b);
    fc->key = 0; fc->n = 0;
    // (what this cache holds now is given back first -- by the thread, where a thread allocates)
    std::vector<double*> give_back;
    if (g.replace) { give_back.swap(fc->blocks); fc->block_rows = 0; }
    if (g.in_thread) {
        frozen_request(fc, c->dev, pl, g, give_back);
        return 1;
    }
    for (double* p : give_back) (void)hipFree(p);
    std::vector<double*> got;
    NK2D_CHECK(c, frozen_alloc_blocks(g.count, g.block_bytes, &got));
    frozen_take_blocks(c, fc, pl, g, &got);
    return 0;
}

// everything the build writes to: the one-off planes, the blocks, the row arrays (the slab: with its head-room), the pieces' bases
static int frozen_ensure_storage(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenPlanIn& in, const FrozenPlan& pl, int64_t n) {
    if (pl.lean) NK2D_TRY(frozen_grow(c, (void**)&fc->lean_tab, &fc->lean_tab_doubles, 3 * in.nv + 3 * frozen_ntab(in), sizeof(double)));
    if (pl.src || pl.phos) NK2D_TRY(frozen_grow(c, (void**)&fc->upr, &fc->upr_doubles, pl.phos ? in.np : in.nv, sizeof(double)));   // (phosphorus: one plane, d uptake / d po4)
    NK2D_TRY(frozen_ensure_blocks(c, fc, in, pl, n));
    const size_t rows_want = pl.pieces ? (size_t)n : fc->block_rows;
    if (fc->rows_cap < rows_want) {
        size_t cap_r = fc->rows_cap, cap_f = fc->rows_cap;
        fc->rows_cap = 0;
        NK2D_TRY(frozen_grow(c, (void**)&fc->rows_dev, &cap_r, rows_want, sizeof(CacheRow)));
        NK2D_TRY(frozen_grow(c, (void**)&fc->frows_dev, &cap_f, rows_want, sizeof(FrozenRow)));
        fc->rows_cap = rows_want;
    }
    if (pl.pieces) {
        NK2D_TRY(frozen_grow(c, (void**)&fc->blocks_dev, &fc->blocks_dev_cap, fc->blocks.size(), sizeof(double*)));
        NK2D_CHECK(c, hipMemcpy(fc->blocks_dev, fc->blocks.data(), sizeof(double*) * fc->blocks.size(), hipMemcpyHostToDevice));
    }
    return 0;
}

// CachePtrs -- the slab flavour's tables, and the sizes either flavour reads -- and PieceTab -- the piece flavour's -- from the one
// layout.  A lean cache's six factor tables are the one row `lean_tab`; a cache in pieces has no table pointers
static CachePtrs frozen_cache_ptrs(const nk2d_frozen_cache* fc, const FrozenLayout& L) {
    CachePtrs C = {};
    C.kv_len = L.kv_len; C.np = L.np; C.nv = L.nv; C.ntab = L.ntab;
    double* b = fc->pieces ? nullptr : fc->blocks[0];
    if (b) { C.KV = b; C.J = b + L.oJ; }
    if (L.lean) {
        double* p = fc->lean_tab;
        C.fr_inv = p; C.fc_invr = p + L.nv; C.fc_invi = p + 2 * L.nv;
        p += 3 * L.nv;
        C.fr_tab = p; C.fc_tabr = p + L.ntab; C.fc_tabi = p + 2 * L.ntab;
    } else if (b) {
        C.fr_inv = b + L.ofr; C.fc_invr = b + L.ofcr; C.fc_invi = b + L.ofci;
        C.fr_tab = b + L.otr; C.fc_tabr = b + L.otcr; C.fc_tabi = b + L.otci;
    }
    return C;
}
static PieceTab frozen_piece_tab(const nk2d_frozen_cache* fc, const FrozenLayout& L) {
    PieceTab T;
    T.base = fc->blocks_dev;
    T.rows = (int)L.B;
    T.oJ = L.oJ; T.ofr = L.ofr; T.ofcr = L.ofcr; T.ofci = L.ofci; T.otr = L.otr; T.otcr = L.otcr; T.otci = L.otci;
    T.oS = L.oS;
    return T;
}

// the rows of the schedule as the build kernels (CacheRow: times, forcing, where the row's planes go) and the year (FrozenRow) read them
static void frozen_fill_rows(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenLayout& L, const double* sched, int64_t n, std::vector<CacheRow>* rows) {
    const double RCs[3] = {0.15505102572168222, 0.6449489742783178, 1.0};
    const double MU_REAL = 3.637834252744496, MU_CR = 2.6810828736277523, MU_CI = -3.050430199247411;
    auto at = [&](int64_t i, int slot) {
        const FrozenPlace p = frozen_place(L, (size_t)i, slot);
        return fc->blocks[p.block] + p.offset;
    };
    rows->assign((size_t)n, CacheRow());
    fc->frows.assign((size_t)n, FrozenRow());
    for (int64_t i = 0; i < n; ++i) {
        const double* r = sched + i * NK2D_SCHED_WIDTH;
        const double t = r[0], t_new = r[1], h = r[2], t_jac = r[4], h_lu = r[5];
        CacheRow& R = (*rows)[(size_t)i];
        double times[4];
        for (int k = 0; k < 3; ++k) times[k] = t + (h * RCs[k]);
        times[3] = t_jac;
        for (int k = 0; k < 4; ++k) {
            nk2d_host_interp(4, c->d.bld_tvals, c->d.bld_fvals, times[k], &R.v.frac[k]);
            R.v.out[k] = (k < 3) ? at(i, FROZEN_KV0 + k) : nullptr;
        }
        // (slot 3 of a thresholded forced module: where the file source at the Jacobian time goes)
        if (L.src) R.v.out[3] = at(i, FROZEN_SRC);
        vmix_forcing_args(c, L.src ? 4 : 3, times, R.v);
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
}

// planes and Jacobian of every row, and -- a full cache -- its line factorisations: the work of two kernels
template <int PIECES>
static int frozen_build_tables(nk2d_ctx* c, const CacheRow* rows_dev, typename CacheArgOf<PIECES>::type C, int64_t n, bool lean) {
    DevP P = make_devp(c);
    const long long tasks = 4LL * c->ny * n;
    NK2D_DISPATCH_E(c->E, hipLaunchKernelGGL((k_cache_planes<EE, PIECES>), dim3((unsigned)((tasks + 3) / 4)), dim3(NK2D_BLOCK), 0, nk2d_s(c),
                                              P, rows_dev, C, (int)n));
    NK2D_CHECK(c, hipGetLastError());
    c->st.nlaunch += 1;
    if (lean) return 0;
    const long long ftasks = 2LL * c->ncol * n;
    NK2D_DISPATCH_EK(c->E, c->kind, hipLaunchKernelGGL((k_cache_factor<EE, KK, PIECES>), dim3((unsigned)((ftasks + 3) / 4)), dim3(NK2D_BLOCK), 0,
                                                       nk2d_s(c), P, rows_dev, C, (int)n));
    NK2D_CHECK(c, hipGetLastError());
    c->st.nlaunch += 1;
    return 0;
}

// (re)build the cache for this schedule
static int frozen_build(nk2d_ctx* c, nk2d_frozen_cache* fc, const FrozenPlanIn& in, const FrozenPlan& pl, const double* sched, int64_t n) {
    const FrozenLayout L = frozen_layout(in, fc->block_rows, fc->lean, fc->src);
    std::vector<CacheRow> rows;
    frozen_fill_rows(c, fc, L, sched, n, &rows);
    NK2D_CHECK(c, hipMemcpyAsync(fc->rows_dev, rows.data(), sizeof(CacheRow) * (size_t)n, hipMemcpyHostToDevice, nk2d_s(c)));
    NK2D_CHECK(c, hipMemcpyAsync(fc->frows_dev, fc->frows.data(), sizeof(FrozenRow) * (size_t)n, hipMemcpyHostToDevice, nk2d_s(c)));
    NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));    // `rows` leaves scope
    if (pl.pieces) {
        CachePiecePtrs CP;
        CP.C = frozen_cache_ptrs(fc, L);
        CP.T = frozen_piece_tab(fc, L);
        NK2D_TRY(frozen_build_tables<1>(c, fc->rows_dev, CP, n, pl.lean));
    } else {
        NK2D_TRY(frozen_build_tables<0>(c, fc->rows_dev, frozen_cache_ptrs(fc, L), n, pl.lean));
    }
    fc->key = pl.key;
    fc->n = n;
    c->frozen_cache_builds++;
    return 0;
}

// the store holds the plan's form, and -- a cache in pieces -- every piece that covers rows < n is there: the kernel never looks
// at a missing one
static bool frozen_holds(const nk2d_frozen_cache* fc, const FrozenPlan& pl) {
    if (fc->pieces != pl.pieces || fc->lean != pl.lean || fc->src != pl.src || fc->blocks.empty()) return false;
    if (!pl.pieces) return true;
    if (fc->block_rows != pl.B || fc->blocks.size() < pl.need || !fc->blocks_dev || fc->blocks_dev_cap < pl.need) return false;
    for (size_t p = 0; p < pl.need; ++p)
        if (!fc->blocks[p]) return false;
    return true;
}

// the year's own device buffers (first use)
static int frozen_year_buffers(nk2d_ctx* c) {
    if (c->YR_OUT) return 0;
    NK2D_CHECK(c, hipMalloc((void**)&c->YR_PART, sizeof(double) * 2 * c->ncol));
    NK2D_CHECK(c, hipMalloc((void**)&c->YR_OUT, sizeof(double) * 32));
    // (behind the synchronisation block: U and UN of the stage-value exchange, option "frozen_stage_exchange")
    NK2D_CHECK(c, hipMalloc((void**)&c->YR_SYNC, yr_sync_bytes(c) + yr_xchg_bytes(c)));
    NK2D_CHECK(c, hipMalloc((void**)&c->YR_MTAB, sizeof(int) * std::max<size_t>(c->rho_tab.size(), 1)));
    NK2D_CHECK(c, hipHostMalloc((void**)&c->hYR_OUT, sizeof(double) * 32));
    NK2D_CHECK(c, hipEventCreate(&c->yr_ev[0]));
    NK2D_CHECK(c, hipEventCreate(&c->yr_ev[1]));
    c->yr_lin_tol = -1.0;
    c->yr_rec_cap = 0;
    c->YR_REC = nullptr;
    return 0;
}

// the kernel's arguments (the slab flavour takes the FrozenArgs part)
static int frozen_year_args(nk2d_ctx* c, const nk2d_frozen_cache* fc, const FrozenPlanIn& in, const FrozenPlan& pl, int64_t n, DevP* P, FrozenPieceArgs* Ap) {
    const FrozenLayout L = frozen_layout(in, fc->block_rows, fc->lean, fc->src);
    FrozenPieceArgs& A = *Ap;
    A = {};
    if (pl.pieces) A.T = frozen_piece_tab(fc, L);
    A.Y = c->Y; A.YOLD = c->YOLD; A.Z = c->Z; A.ZN = c->ZN; A.W = c->W; A.F = c->F;
    A.BR = c->BR; A.BCR = c->BCR; A.BCI = c->BCI;
    for (int i = 0; i < 2; ++i) { A.XR[i] = c->XR[i]; A.XCR[i] = c->XCR[i]; A.XCI[i] = c->XCI[i]; }
    A.PART = c->YR_PART;
    A.STEP_PART = c->STEP_PART;
    A.rows = fc->frows_dev;
    A.C = frozen_cache_ptrs(fc, L);
    A.n = (int)n;
    A.arrive = (unsigned*)c->YR_SYNC; A.abort_flag = (int*)((char*)c->YR_SYNC + 4096);
    A.out = c->YR_OUT;
    A.spin_ticks = (long long)(c->barrier_timeout_ms * 1.0e5);
    A.fences = c->year_fences;
    // a thresholded forced module: the year forms UPR, in the cache's own plane, from the rows' source planes
    // (phosphorus: from the state and the context's light plane alone.  A year that is handed back leaves the context's own UPR what the
    // launch path left there)
    A.upr_on = (pl.src || pl.phos) ? 1 : 0;
    A.SRC = (pl.src && !pl.pieces) ? fc->blocks[0] + L.oS : nullptr;
    *P = make_devp(c);
    if (pl.src || pl.phos) P->UPR = fc->upr;
    NK2D_TRY(frozen_fit_lds(c, in, pl, &A.coef_lds, &A.by_column));
    c->frozen_lds_bits = A.coef_lds;
    c->frozen_early_bits = (A.coef_lds & 48) == 48 ? c->frozen_early : 0;   // (48 is there only where the own state is compiled in: frozen_lds_shape)
    // (invariant: bit 8 only together with bits 0 - 5.  Everything that takes A.coef_lds from here on -- frozen_lds_doubles() in the
    // launch functions, the kernel -- tests bits below 64 or non-zero, which bit 8 on top of 63 does not change)
    A.coef_lds |= c->frozen_early_bits << 8;
    // option "frozen_stage_exchange", bit 9, under the same rule.  It changes no decision: not part of the schedule fingerprint
    // (and only in the instantiations that have the body for it: NK2D_FROZEN_XCHG)
    const bool team_year = c->frozen_team && c->E <= 2 && !pl.phos;
    c->frozen_stage_exchange_bits =
        ((A.coef_lds & 48) == 48 && NK2D_FROZEN_XCHG(c->E, c->kind, team_year, pl.pieces, pl.lean)) ? c->frozen_stage_exchange : 0;
    A.coef_lds |= c->frozen_stage_exchange_bits << 9;
    // option "frozen_xlane", bit 10, only on top of bit 9 and in the instantiations that have the body (NK2D_FROZEN_XLANE): no decision,
    // not part of the schedule fingerprint either
    c->frozen_xlane_bits =
        (c->frozen_stage_exchange_bits != 0 && NK2D_FROZEN_XLANE(c->E, c->kind, team_year, pl.pieces, pl.lean)) ? c->frozen_xlane : 0;
    A.coef_lds |= c->frozen_xlane_bits << 10;
    // option "frozen_dedicated": where all of the above say CL 959, the entry that carries that body alone (frozen_dedicated(): the rule;
    // frozen_launch_year() takes it from the counter).  Bit 11, read by that entry only: its hand-over polls with one load.  No
    // decision, not part of the schedule fingerprint or the cache key
    c->frozen_dedicated_bits = frozen_dedicated(c->frozen_dedicated, c->E, c->kind, team_year, pl.pieces, pl.lean, c->frozen_lds_bits,
                                                c->frozen_early_bits, c->frozen_stage_exchange_bits, c->frozen_xlane_bits);
    if (c->frozen_dedicated_bits == 2) A.coef_lds |= 1 << 11;
    return 0;
}

// the year: one launch, waited for.  2: a wait inside the kernel timed out
static int frozen_launch_year(nk2d_ctx* c, const FrozenPlan& pl, int64_t n, DevP& P, FrozenPieceArgs& A) {
    // option "frozen_team": a workgroup per column (four waves: newton_team_body) instead of a wave per column, up to two levels per
    // lane.  Measured in round 3 (profiles/r03_frozen_team.log, r03_frozen_nbsync.log): teams want a CU each and beat the
    // wave-per-column year at every such size -- 26^2 9.4 ms, 52^2 14.9, 104^2 27.0 with the neighbour hand-over.
    // (a phosphorus year at those depths -- option "frozen_phosphorus_shallow" -- is one ypos column to a workgroup: no team)
    const bool team = c->frozen_team && c->E <= 2 && !pl.phos;
    const dim3 grid((unsigned)(team ? c->ncol : nk2d_grid(c->ncol)));
    NK2D_CHECK(c, hipMemsetAsync(c->YR_SYNC, 0, yr_sync_bytes(c), nk2d_s(c)));
    NK2D_CHECK(c, hipMemsetAsync(c->YR_OUT, 0, sizeof(double) * 32, nk2d_s(c)));
    NK2D_CHECK(c, hipEventRecord(c->yr_ev[0], nk2d_s(c)));
    {
        // one resident kernel at a time in this process (the turn is held until this one has ended)
        struct Turn {
            int waves;
            explicit Turn(int w) : waves(w) { nk2d_turn_take(waves); }
            ~Turn() { nk2d_turn_give(waves); }
        } turn(team ? 4 * c->ncol : c->ncol);
        hipError_t rc = hipErrorInvalidValue;
        bool two = false;
        if (c->frozen_dedicated_bits != 0) rc = launch_resident_dedicated(c, pl.pieces, P, A);
        else if (pl.phos) rc = launch_frozen_phos_flavour(c, pl.pieces, P, A, false, &two);
        else if (pl.lean) rc = pl.pieces ? launch_frozen<1, 1>(c, team, grid, P, A) : launch_frozen<0, 1>(c, team, grid, P, static_cast<FrozenArgs&>(A));
        else rc = pl.pieces ? launch_frozen<1, 0>(c, team, grid, P, A) : launch_frozen<0, 0>(c, team, grid, P, static_cast<FrozenArgs&>(A));
        c->frozen_two_waves_last = two ? 1 : 0;
        if (rc == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return 1; }
        NK2D_CHECK(c, rc);
        NK2D_CHECK(c, hipEventRecord(c->yr_ev[1], nk2d_s(c)));
        NK2D_CHECK(c, hipMemcpyAsync(c->hYR_OUT, c->YR_OUT, sizeof(double) * 32, hipMemcpyDeviceToHost, nk2d_s(c)));
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
    }
    const double* o = c->hYR_OUT;
    if ((int)o[0] != 0 || (int64_t)o[1] != n) return 2;
#ifdef NK2D_FROZEN_CLOCKS
    std::fprintf(stderr, "frozen clocks (early %d, stage exchange %d, xlane %d): %.0f phases, per phase drain %.3f us, flag store to poll match %.3f us, "
                 "poll match to neighbours loaded %.3f us, rest %.3f us; kernel %.3f ms\n",
                 c->frozen_early_bits, c->frozen_stage_exchange_bits, c->frozen_xlane_bits, o[11], 0.01 * o[8] / o[11], 0.01 * o[9] / o[11], 0.01 * o[12] / o[11],
                 0.01 * (o[10] - o[8] - o[9] - o[12]) / o[11], 1.0e-5 * o[10]);
#endif
    if (team) c->frozen_team_years++;
    // the launch itself, between two events on the context's stream (bench.py's roofline of the one-launch year)
    float ms = 0.f;
    NK2D_CHECK(c, hipEventElapsedTime(&ms, c->yr_ev[0], c->yr_ev[1]));
    c->frozen_launch_us += (int64_t)(1000.0 * (double)ms);
    if ((int)o[2]) std::swap(c->Y, c->YOLD);
    if ((int)o[3]) std::swap(c->Z, c->ZN);
    return 0;
}

// counters of the year, as the launch-per-phase path books them, and the algorithmic bytes of its phases (the formula of
// the launches they replace; nothing of the schedule cache's one-off construction)
static void frozen_book_year(nk2d_ctx* c, const nk2d_frozen_cache* fc, int64_t n, std::vector<char>* err_rows) {
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
}

// 0: the year ran in one launch (buffers in their roles after the last-but-one row's end; the last row's Newton iterations
//    done, its commit left to the caller);  1: not for this context / schedule (the launch-per-phase path runs);
// 2: a grid barrier timed out (the same);  < 0: error
int nk2d_frozen_persistent(nk2d_ctx* c, const double* sched, int64_t n, std::vector<char>* err_rows) {
    const FrozenPlanIn in = frozen_plan_in(c);
    if (!frozen_eligible(in, sched, n)) return 1;
    FrozenPlan pl;
    NK2D_TRY(frozen_make_plan(c, in, sched, n, &pl));
    if (pl.phos) NK2D_TRY(frozen_phos_resident(c, in, pl));
    nk2d_frozen_cache* fc = frozen_store(c);
    NK2D_TRY(frozen_thread_done(c, fc));
    NK2D_TRY(frozen_drop_other_form(c, fc, pl));
    NK2D_TRY(frozen_admitted(c, in, pl, n));
    if (fc->key != pl.key || fc->n != n) {
        NK2D_TRY(frozen_deferred(c, in, pl));
        NK2D_TRY(frozen_ensure_storage(c, fc, in, pl, n));
        NK2D_TRY(frozen_build(c, fc, in, pl, sched, n));
    }
    if (!frozen_holds(fc, pl)) return 1;
    NK2D_TRY(frozen_year_buffers(c));
    DevP P;
    FrozenPieceArgs A;
    NK2D_TRY(frozen_year_args(c, fc, in, pl, n, &P, &A));
    NK2D_TRY(frozen_launch_year(c, pl, n, P, A));
    frozen_book_year(c, fc, n, err_rows);
    return 0;
}

// Options "frozen_cache_pieces" + "frozen_cache_early": the pieces for the `n` rows of the schedule a free-running year just
// recorded are asked for NOW, from the thread whatever their size, so that they are there when the first product comes; the
// tables are built where they always are, at the first frozen year.  Pieces are what makes the request one the driver can serve
// beside other allocations -- or not: DESIGN 3.6.
// (Asking for the SLAB earlier -- at the end of the free-running year whose steps the products will repeat -- was built and
// measured in round 4 and taken out again: in a fresh process the hipMalloc of 120 GB holds the driver for ~ 4 s, and the
// preconditioner's set-up, which lies between F(x) and the first product and allocates its 10 GB of inverses, waited behind it:
// set-up 0.50 -> 4.18 s, spin-up of iage 416 x 416 3.98 / 5.14 -> 9.34 s (profiles/r04_prealloc_experiment.log).  Beside the first
// products, which allocate nothing, the same request costs them 0.1 - 1.2 s in all.)
int nk2d_frozen_cache_early(nk2d_ctx* c, const double* sched, int64_t n) {
    if (!c->frozen_cache_pieces || !c->frozen_cache_early || !sched) return 0;
    const FrozenPlanIn in = frozen_plan_in(c);
    if (!frozen_eligible(in, sched, n)) return 0;
    // (a step's 1 -- nothing to ask for -- is no error here)
    auto quiet = [](int rc) { return rc < 0 ? rc : 0; };
    FrozenPlan pl;
    int rc = frozen_make_plan(c, in, sched, n, &pl);
    if (rc) return quiet(rc);
    nk2d_frozen_cache* fc = frozen_store(c);
    if ((rc = frozen_thread_done(c, fc)) != 0) return quiet(rc);
    NK2D_TRY(frozen_drop_other_form(c, fc, pl));
    const FrozenHeld held = frozen_held(c);
    if (!frozen_must_grow(pl, held, n)) return 0;
    if ((rc = frozen_admitted(c, in, pl, n)) != 0) return quiet(rc);
    frozen_request(fc, c->dev, pl, frozen_growth(in, pl, held, n, 0.0), {});
    c->frozen_cache_early_requests++;
    return 0;
}
