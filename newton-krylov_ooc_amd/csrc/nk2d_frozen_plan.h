// nk2d_frozen_plan.h -- the arithmetic of the schedule cache of the one-launch frozen year (nk2d_frozen.hip): whether a schedule is
// eligible, which form its cache takes, what it may cost, how it grows, where row i's tables lie and what of a column lives in
// LDS.  Pure host C++, no HIP types, each rule written once: `make -C csrc asan-host` compiles tests/host_asan/test_frozen_plan.cpp
// against this header with a plain g++ under -fsanitize=address,undefined and runs it on the CPU.  Whatever asks the device
// (hipMemGetInfo, the compute-unit count) stays with the caller and comes in as an argument.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

// (the library's own constants, token for token as nk2d_common.h, nk2d_bodies.h and include/nk2d.h define them: a value that
// drifts there is a redefinition the compiler reports where both are seen)
#define NK2D_WAVES_PER_BLOCK 4
#define NK2D_TAB 14
#define NK2D_SCHED_WIDTH 8
#define NK2D_COEF_LDS_DOUBLES(E) ((7 * (E) + 1) * 64)

// A column's own state from phase to phase (OwnState, bits 16 and 32 of option "frozen_coef_lds"): the instantiations of
// k_frozen_persistent that carry it.  A wave per column by column, the linear-source kinds, the full cache, five to seven levels
// per lane: the lean factorising phase and phosphorus keep their bodies, and at eight levels per lane neither the registers (421
// of 512 before, one of them spilled) nor the LDS of a compute unit with two workgroups hold it
// (profiles/r09_frozen_own_state_resources.log).  The kernel and frozen_lds_shape() read this one macro.
#define NK2D_FROZEN_OWN(E, KIND, TEAM, LEAN) ((E) >= 5 && (E) <= 7 && ((KIND) == 0 || (KIND) == 2) && !(TEAM) && !(LEAN))
// ... and of those the ones whose waves may exchange stage values with their neighbours (option "frozen_stage_exchange"): all but the
// piece flavour of the linear-source kind at seven levels per lane, where the body with the exchange beside the others makes the
// compiler report a spilled register (<7, 0, 0, 1, 0>: that class stays on the body without it)
#define NK2D_FROZEN_XCHG(E, KIND, TEAM, PIECES, LEAN) (NK2D_FROZEN_OWN(E, KIND, TEAM, LEAN) && !((E) == 7 && (KIND) == 0 && (PIECES)))
// ... and of those the ones that carry the body whose cross-lane moves go through the VALU (option "frozen_xlane"; the moves
// themselves: NK2D_FROZEN_XLANE_MOVES in nk2d_common.h): all but the piece flavour of the linear-source kind at six levels per
// lane, where that body beside the others makes the compiler report a spilled register (<6, 0, 0, 1, 0>)
#define NK2D_FROZEN_XLANE(E, KIND, TEAM, PIECES, LEAN) (NK2D_FROZEN_XCHG(E, KIND, TEAM, PIECES, LEAN) && !((E) == 6 && (KIND) == 0 && (PIECES)))
// The instantiations of k_frozen_persistent_d (nk2d_frozen_d.hip), the entry that carries the body of the default year alone (CL 959:
// everything in LDS, the whole own state, "frozen_early", the stage-value exchange, the VALU moves): those NK2D_FROZEN_XLANE names
// for a wave per column on the full cache
#define NK2D_FROZEN_DEDICATED(E, KIND, PIECES) NK2D_FROZEN_XLANE(E, KIND, 0, PIECES, 0)

// Option "frozen_dedicated" (0: k_frozen_persistent; 1: the dedicated entry with today's hand-over; 2: with the one-load poll) as in
// effect in a year: the dedicated entry is taken only where the year would run CL 959 in k_frozen_persistent -- every part of the
// column in LDS and the own state (`lds_bits` 63, which frozen_lds_shape() grants by column only), and "frozen_early", the stage-value
// exchange and the VALU moves in effect (each 0 where its instantiation has no body for it) -- and the entry has the instantiation
static inline int frozen_dedicated(int option, int E, int kind, bool team, bool pieces, bool lean, int lds_bits, int early_bits,
                                   int stage_exchange_bits, int xlane_bits) {
    if (option != 1 && option != 2) return 0;
    if (team || lean || !NK2D_FROZEN_DEDICATED(E, kind, pieces ? 1 : 0)) return 0;
    if (lds_bits != 63 || early_bits != 1 || stage_exchange_bits != 1 || xlane_bits != 1) return 0;
    return option;
}

// what of a context (nk2d_ctx) and its options the cache's arithmetic reads
struct FrozenPlanIn {
    int E, kind, tc, ny, ncol;
    size_t np, nv, kv_len;
    int sms_nrec;
    double sink_thres, t0;
    int frozen_persistent, frozen_persistent_max_e, frozen_forced, frozen_phosphorus;
    int frozen_phosphorus_shallow;
    int frozen_cache_lean, frozen_cache_pieces;
    double frozen_cache_piece_mb;
    int64_t frozen_cache_piece_rows;
    double frozen_cache_max_gb;
    int frozen_cache_after, frozen_alloc_async, frozen_err_check;
    int frozen_coef_lds, frozen_by_column, frozen_wpb, frozen_team;
    int factor_fp32, jac_stage_state, hist_n;
    bool norm_hook;
};

// what a context's cache holds right now: `blocks` device blocks of `block_rows` rows each (a slab is ONE block, pieces == false),
// in one form (lean: the planes only; src: and the file-source planes); `alloc_state` / `alloc_lean`: what a thread is allocating
struct FrozenHeld {
    bool pieces = false, lean = false, src = false;
    size_t blocks = 0, block_rows = 0;
    int alloc_state = 0;
    bool alloc_lean = false;
    uint64_t key = 0;
    int64_t n = 0;
    size_t rows() const { return blocks * block_rows; }
};

// a forced module whose file source has a sink threshold: its Jacobian reads the state (the diagonal plane UPR)
static inline bool frozen_thres(const FrozenPlanIn& in) { return in.kind == 2 && in.sms_nrec > 0 && in.sink_thres > 0.0; }

// phosphorus (module_kind 1) where option "frozen_phosphorus" lets it take the one-launch year: on the lean cache ("frozen_cache_lean" 1, or
// 2, which for such a context always means lean), at three to eight levels per lane -- the workgroup is then one ypos column with
// its tracers, a wave each.  One and two levels per lane come in with option "frozen_phosphorus_shallow" only: the same by-column
// workgroup with nothing of the year in LDS (the four-wave teams of those depths cannot hold three coupled tracers: no team there)
static inline bool frozen_phos(const FrozenPlanIn& in) {
    const int e_min = in.frozen_phosphorus_shallow != 0 ? 1 : 3;
    return in.kind == 1 && in.frozen_phosphorus != 0 && in.frozen_cache_lean != 0 && in.E >= e_min && in.E <= 8 && in.tc <= NK2D_WAVES_PER_BLOCK;
}

static inline size_t frozen_ntab(const FrozenPlanIn& in) { return (size_t)in.ncol * NK2D_TAB * 64; }

// doubles of a row of the cache (lean: the planes only; src: and the file-source plane at the Jacobian time)
static inline size_t frozen_row_doubles(const FrozenPlanIn& in, bool lean, bool src) {
    return 3 * in.kv_len + 5 * in.np + (lean ? 0 : 3 * in.nv + 3 * frozen_ntab(in)) + (src ? in.np : 0);
}

// rows per piece: option "frozen_cache_piece_rows", or what fits "frozen_cache_piece_mb" MiB (at least one)
static inline size_t frozen_piece_rows(const FrozenPlanIn& in, bool lean, bool src) {
    if (in.frozen_cache_piece_rows > 0) return (size_t)in.frozen_cache_piece_rows;
    const double fit = std::floor(in.frozen_cache_piece_mb * 1048576.0 / (8.0 * (double)frozen_row_doubles(in, lean, src)));
    return fit >= 1.0 ? (size_t)std::min(fit, 1.0e9) : (size_t)1;
}

// bytes of HBM the held cache takes
static inline double frozen_held_bytes(const FrozenPlanIn& in, const FrozenHeld& h) {
    return 8.0 * (double)h.rows() * (double)frozen_row_doubles(in, h.lean, h.src);
}

// never more than what the device has to spare right now (other contexts of the process, other tenants): a cache of `bytes`
// is admitted where, with 2 % on top, it stays within 85 % of what is free plus what this cache already holds
static inline bool frozen_admit(double bytes, double free_bytes, double held_bytes) { return !(1.02 * bytes > 0.85 * (free_bytes + held_bytes)); }

// ---- is the one-launch year made for this context and schedule?
static inline bool frozen_eligible(const FrozenPlanIn& in, const double* sched, int64_t n) {
    // a Jacobian that reads the state: a forced module with a thresholded sink with option "frozen_forced" bit 2, phosphorus with
    // option "frozen_phosphorus" -- both on the lean cache only (their full cache -- factorisations ahead of the state -- cannot exist)
    const bool thres = frozen_thres(in);
    const bool phos = frozen_phos(in);
    const bool needs_state = (in.kind == 1 && !phos) || (thres && !((in.frozen_forced & 2) && in.frozen_cache_lean != 0));
    if (!in.frozen_persistent || needs_state || in.hist_n != 0 || in.norm_hook || n < 1) return false;
    // the cache holds the factorisation in double precision only: with option "factor_fp32" the recorded year read the single
    // precision copies, and the one-launch year would not be the same discrete map (round-3 ADVICE) -- launch by launch then
    if (in.factor_fp32) return false;
    // (one to four levels per lane; five to eight with linear sources -- for the file-driven forced module there with option
    // "frozen_forced": bit 1 without, bit 2 with a sink threshold)
    if (in.E > in.frozen_persistent_max_e || in.E > 8) return false;
    if (in.E > 4 && in.kind != 0 && !phos && !(in.kind == 2 && (in.frozen_forced & (thres ? 2 : 1)))) return false;
    if (thres || phos) {
        // UPR is formed where the launch path evaluates the Jacobian anew (replay_rows): at a step start, or -- option
        // "jac_stage_state" -- at a stage time of the row's own attempt.  A schedule it would refuse goes to it, to be refused
        const double RCs[3] = {0.15505102572168222, 0.6449489742783178, 1.0};
        double t_jac_prev = in.t0;
        for (int64_t i = 0; i < n; ++i) {
            const double* r = sched + i * NK2D_SCHED_WIDTH;
            const double t = r[0], h = r[2], t_jac = r[4];
            if (t_jac != t_jac_prev && t_jac != t) {
                bool at_stage = false;
                for (int k = 0; k < 3 && in.jac_stage_state; ++k) at_stage = at_stage || t_jac == t + (h * RCs[k]);
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

// ---- what a schedule cache (and a command tape, option "frozen_tape") is kept for: the schedule, the context's fingerprint and
// the error-estimate stride (the rows also say which steps carry an error estimate) ...
static inline uint64_t frozen_sched_hash(const double* sched, int64_t n) {
    uint64_t h = 14695981039346656037ull;
    const unsigned char* p = (const unsigned char*)sched;
    const size_t nb = sizeof(double) * (size_t)n * NK2D_SCHED_WIDTH;
    for (size_t i = 0; i < nb; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h ? h : 1;
}
static inline uint64_t frozen_key_full(const FrozenPlanIn& in, uint64_t sched_hash, uint64_t fingerprint) {
    return sched_hash ^ fingerprint ^ ((uint64_t)(in.frozen_err_check + 1) * 0x9E3779B97F4A7C15ull);
}
// ... and the form: a LEAN cache of the same schedule has another key (a full cache is never read as a lean one); so has a lean
// cache with the file-source planes of option "frozen_forced" bit 2, and the lean cache of a phosphorus context
static const uint64_t FROZEN_LEAN_KEY = 0xC2B2AE3D27D4EB4Full;
static const uint64_t FROZEN_SRC_KEY = 0x165667B19E3779F9ull;
static const uint64_t FROZEN_PHOS_KEY = 0x27D4EB2F165667C5ull;
static inline uint64_t frozen_form_key(uint64_t key_full, bool lean, bool src, bool phos) {
    return key_full ^ (lean ? FROZEN_LEAN_KEY : 0) ^ (src ? FROZEN_SRC_KEY : 0) ^ (phos ? FROZEN_PHOS_KEY : 0);
}

// ---- the form of the cache of a schedule of `n` rows (option "frozen_cache_lean"; key_full: its key as a full cache).  0: full,
// 1: lean, 2: lean only where the full cache would be refused -- by "frozen_cache_gb", or by the 85 % rule where it would have to
// be allocated.  What a thread is allocating stays what it is, and so does a lean cache the 85 % rule chose for this very
// schedule (`lean_mem_key`: the schedule it refused last -- the device is not asked again every year); "frozen_cache_gb" is
// looked at every time.  Returns 1 lean, 0 full, -1: the 85 % rule decides and `free_bytes` is needed (asked with nullptr: the
// caller asks the device and comes again).  *ruled: that rule made the decision (the caller remembers the schedule)
static inline int frozen_form(const FrozenPlanIn& in, int64_t n, uint64_t key_full, const FrozenHeld& held, uint64_t lean_mem_key,
                              const double* free_bytes, bool* ruled) {
    *ruled = false;
    if (frozen_thres(in) || in.kind == 1) return 1;     // (eligible with a lean cache only: "frozen_cache_lean" 2 always means lean here)
    if (in.frozen_cache_lean != 2) return in.frozen_cache_lean == 1 ? 1 : 0;
    if (held.alloc_state != 0) return held.alloc_lean ? 1 : 0;
    const bool pieces = in.frozen_cache_pieces != 0;
    const size_t B = pieces ? frozen_piece_rows(in, false, false) : 1, rows = ((size_t)n + B - 1) / B * B;
    const double bytes = 8.0 * (double)rows * (double)frozen_row_doubles(in, false, false);
    if (bytes > in.frozen_cache_max_gb * 1.0e9) return 1;
    const bool holds = held.blocks != 0;
    if (holds && !held.lean && held.pieces == pieces) {     // (room enough in the full form already: nothing to allocate, nothing to refuse)
        if (pieces ? (held.block_rows == B && held.rows() >= rows) : held.rows() >= (size_t)n) return 0;
    }
    if (holds && held.lean && held.n == n && held.key == (key_full ^ FROZEN_LEAN_KEY) && lean_mem_key == key_full) return 1;
    if (!free_bytes) return -1;
    *ruled = true;
    return frozen_admit(bytes, *free_bytes, frozen_held_bytes(in, held)) ? 0 : 1;
}

// ---- the cache a schedule of n rows asks for
struct FrozenPlan {
    bool pieces, lean, src, phos;
    size_t per_row;      // doubles of a row in this form
    size_t B, need;      // pieces: `need` blocks of `B` rows (the slab: 0, 0)
    double bytes;        // what the limits apply to: the sum of the pieces; of the slab, the n rows
    bool allowed;        // option "frozen_cache_gb"
    uint64_t key;
};
static inline FrozenPlan frozen_plan(const FrozenPlanIn& in, int64_t n, uint64_t key_full, bool lean) {
    FrozenPlan pl;
    pl.pieces = in.frozen_cache_pieces != 0;
    pl.lean = lean;
    // (a thresholded forced module -- eligible with option "frozen_forced" bit 2 only, and lean: a row holds its source plane too)
    pl.src = frozen_thres(in);
    // (phosphorus -- eligible with option "frozen_phosphorus" only, and lean: a row is KV and J, the light plane is the context's own)
    pl.phos = in.kind == 1;
    pl.per_row = frozen_row_doubles(in, pl.lean, pl.src);
    pl.B = pl.pieces ? frozen_piece_rows(in, pl.lean, pl.src) : 0;
    pl.need = pl.pieces ? ((size_t)n + pl.B - 1) / pl.B : 0;
    pl.bytes = 8.0 * (double)(pl.pieces ? pl.need * pl.B : (size_t)n) * (double)pl.per_row;
    pl.allowed = !(pl.bytes > in.frozen_cache_max_gb * 1.0e9);
    pl.key = frozen_form_key(key_full, pl.lean, pl.src, pl.phos);
    return pl;
}

// a context never holds a slab and pieces at once, nor a full and a lean cache: the other form (and pieces of another size) go first
static inline bool frozen_other_form(const FrozenPlan& pl, const FrozenHeld& held) {
    if (held.blocks == 0) return false;
    return held.pieces != pl.pieces || held.lean != pl.lean || held.src != pl.src || (pl.pieces && held.block_rows != pl.B);
}

// what is held (in the plan's form) does not cover the n rows: storage has to be admitted and allocated
static inline bool frozen_must_grow(const FrozenPlan& pl, const FrozenHeld& held, int64_t n) {
    return pl.pieces ? held.blocks < pl.need : held.rows() < (size_t)n;
}

// option "frozen_cache_after": that many years of a schedule run launch by launch before its cache is built.  Default 0; -1: 0
// for caches below 8 GB, 3 above.  Building a 100 GB cache takes 26 ms where a one-launch year saves 40
// (tools/probe_cache_build.py) -- but its FIRST allocation has been seen to take 0.8 s inside a Newton run, and a Newton
// iteration with two or three Krylov iterations has nothing to pay that back with; a long Krylov solve has.
static inline int frozen_years_before_build(const FrozenPlanIn& in, double bytes) {
    return in.frozen_cache_after >= 0 ? in.frozen_cache_after : (bytes > 8.0e9 ? 3 : 0);
}

// ---- growth: what to allocate, and by whom
struct FrozenGrowth {
    size_t count, block_rows, block_bytes;
    bool replace;        // what is held is given back first (the slab)
    bool in_thread;
};
// The slab: ONE allocation for the whole cache, with room for the longer schedules of later Newton iterates (a sixth more rows
// and 16; within 90 % of what is free plus what the old slab gives back, never below n): giving 100 GB back and asking for them
// again costs seconds (measured inside a Newton run: 4.4 s), the first request 0.03 - 0.8 s.  A slab that is too small is given
// back and replaced.  Pieces: those missing, no headroom rows -- what is there stays where it is.
// Above 8 GB (option "frozen_alloc_async") a thread of the library's own allocates: hipMalloc of 120 GB takes 0.03 - 3 s depending
// on what the process holds on the host and the device, and the years of the meantime run launch by launch.
static inline FrozenGrowth frozen_growth(const FrozenPlanIn& in, const FrozenPlan& pl, const FrozenHeld& held, int64_t n, double free_bytes) {
    FrozenGrowth g;
    g.replace = !pl.pieces;
    if (pl.pieces) {
        g.count = pl.need - held.blocks;
        g.block_rows = pl.B;
    } else {
        const size_t fit = (size_t)(0.9 * (free_bytes + 8.0 * (double)held.rows() * (double)pl.per_row) / (8.0 * (double)pl.per_row));
        g.count = 1;
        g.block_rows = std::max((size_t)n, std::min((size_t)n + (size_t)n / 6 + 16, fit));
    }
    g.block_bytes = sizeof(double) * g.block_rows * pl.per_row;
    g.in_thread = (double)g.count * (double)g.block_bytes > 8.0e9 && in.frozen_alloc_async != 0;
    return g;
}

// ---- ONE layout for both forms: a block of B rows (the slab: B = its capacity) holds, table by table, the rows' KV planes, then
// their J planes, then -- src -- their file-source planes, then -- full -- the six factor tables: the offsets are where each
// table starts inside a block, in doubles (absent tables: 0)
struct FrozenLayout {
    size_t B, kv_len, np, nv, ntab;
    bool lean, src;
    size_t oJ, oS, ofr, ofcr, ofci, otr, otcr, otci;
    size_t block_doubles;
};
enum FrozenSlot { FROZEN_KV0 = 0, FROZEN_KV1, FROZEN_KV2, FROZEN_J, FROZEN_SRC, FROZEN_FR, FROZEN_FCR, FROZEN_FCI, FROZEN_TR, FROZEN_TCR, FROZEN_TCI };
struct FrozenPlace { size_t block, offset; };

static inline FrozenLayout frozen_layout(const FrozenPlanIn& in, size_t B, bool lean, bool src) {
    FrozenLayout L = {};
    L.B = B; L.kv_len = in.kv_len; L.np = in.np; L.nv = in.nv; L.ntab = frozen_ntab(in);
    L.lean = lean; L.src = src;
    size_t o = B * 3 * L.kv_len;
    L.oJ = o; o += B * 5 * L.np;
    if (src) { L.oS = o; o += B * L.np; }
    if (!lean) {
        L.ofr = o; o += B * L.nv;
        L.ofcr = o; o += B * L.nv;
        L.ofci = o; o += B * L.nv;
        L.otr = o; o += B * L.ntab;
        L.otcr = o; o += B * L.ntab;
        L.otci = o; o += B * L.ntab;
    }
    L.block_doubles = o;
    return L;
}

// doubles a slot of one row takes
static inline size_t frozen_slot_doubles(const FrozenLayout& L, int slot) {
    if (slot <= FROZEN_KV2) return L.kv_len;
    if (slot == FROZEN_J) return 5 * L.np;
    if (slot == FROZEN_SRC) return L.np;
    return slot <= FROZEN_FCI ? L.nv : L.ntab;
}

// where slot `slot` of row i lies: the block that holds the row, and the offset inside it
static inline FrozenPlace frozen_place(const FrozenLayout& L, size_t i, int slot) {
    const size_t r = i % L.B;
    const size_t starts[11] = {0, 0, 0, L.oJ, L.oS, L.ofr, L.ofcr, L.ofci, L.otr, L.otcr, L.otci};
    FrozenPlace p;
    p.block = i / L.B;
    p.offset = slot <= FROZEN_KV2 ? (r * 3 + (size_t)slot) * L.kv_len : starts[slot] + r * frozen_slot_doubles(L, slot);
    return p;
}

// ---- what lives in LDS
// doubles of dynamic shared memory of a wave-per-column workgroup of `nwaves` waves (the kernel's layout; bits: LdsSrc)
static inline size_t frozen_lds_doubles(int E, int bits, bool by_column, int nwaves) {
    if (!bits) return 0;
    if (!by_column) return (size_t)nwaves * (NK2D_COEF_LDS_DOUBLES(E) + ((bits & 2) ? 3 * E * 64 : 0));
    return NK2D_COEF_LDS_DOUBLES(E) + ((bits & 4) ? 5 * E * 64 : 0) +
           (size_t)nwaves * (((bits & 2) ? 3 * E * 64 : 0) + ((bits & 8) ? E * 64 : 0) + ((bits & 16) ? E * 64 : 0));
}

// what lives in LDS (option "frozen_coef_lds", bits of LdsSrc) and which columns share a workgroup (option "frozen_by_column"):
// as much as lets a compute unit hold what the grid needs of it -- ceil(workgroups / compute units) of them: pivots, then the step
// block, then W are given up until it fits the 160 KB (E = 8 keeps everything but the pivots).  The column's own state (bits 16:
// Y in LDS, given up before anything else, and 32: the stage values in registers) exists in the instantiations
// NK2D_FROZEN_OWN names, by column, on top of everything else: with a part of 15 missing both bits go; a cache in pieces has
// the stage values only together with Y
static inline void frozen_lds_shape(const FrozenPlanIn& in, bool phos, bool lean, bool pieces, int compute_units, int* coef_lds_out, int* by_column_out) {
    int coef_lds = (in.E >= 3) ? in.frozen_coef_lds : 0;
    // (by column -- and with it the step block and the pivots -- from five levels per lane: 416^2 125.2 -> 120.3 ms; at four the shared
    // block does not pay for the wider hand-over, 208^2 65.2 -> 68.1 ms: profiles/r04_frozen_lds_by_column.log; option value 2 forces it)
    int by_column = (in.frozen_by_column && in.tc <= NK2D_WAVES_PER_BLOCK && coef_lds &&
                     (in.E >= 5 || (in.frozen_by_column >= 2 && in.E >= 3))) ? 1 : 0;
    // (phosphorus: its tracers are coupled inside a ypos column -- by column whatever the two options say, "frozen_coef_lds" 0 included)
    if (phos) by_column = 1;
    if (!by_column) coef_lds &= 3;
    const bool team = in.frozen_team && in.E <= 2 && !phos;     // (a phosphorus year is never a team)
    if (!by_column || phos || (coef_lds & 15) != 15 || !NK2D_FROZEN_OWN(in.E, in.kind, team, lean)) coef_lds &= 15;
    const int nw = by_column ? in.tc : std::max(1, std::min(NK2D_WAVES_PER_BLOCK, in.frozen_wpb));
    const int wgs = by_column ? in.ny : (in.ncol + nw - 1) / nw;
    const int per_cu = (wgs + compute_units - 1) / compute_units;
    for (const int drop : {16, 8, 4, 2}) {
        if (8 * frozen_lds_doubles(in.E, coef_lds, by_column != 0, nw) * (size_t)per_cu <= 160u * 1024u) break;
        coef_lds &= ~drop;
    }
    if ((coef_lds & 15) != 15) coef_lds &= 15;
    if (pieces && (coef_lds & 48) == 32) coef_lds &= 15;      // (the piece flavour has no body for the stage values without Y)
    *coef_lds_out = coef_lds; *by_column_out = by_column;
}
