// The arithmetic of the schedule cache of the one-launch frozen year (csrc/nk2d_frozen_plan.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU: `make -C newton-krylov_ooc_amd/csrc asan-host` (tests/test_host.py runs it).  Known
// answers only, worked out by hand from the rules the header states -- what the GPU tests pin through counters, without a GPU.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "nk2d_frozen_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// tiny sizes: a row is 3 x 5 (KV) + 5 x 4 (J) = 35 doubles lean, + 4 with the source plane, + 3 x 8 + 3 x 1792 = 5400 full
static FrozenPlanIn tiny() {
    FrozenPlanIn in = {};
    in.E = 2; in.kind = 0; in.tc = 1; in.ny = 2; in.ncol = 2;
    in.np = 4; in.nv = 8; in.kv_len = 5;
    in.frozen_persistent = 1; in.frozen_persistent_max_e = 8;
    in.frozen_cache_piece_mb = 1.0; in.frozen_cache_max_gb = 1.0;
    in.frozen_alloc_async = 1; in.frozen_coef_lds = 63; in.frozen_by_column = 1; in.frozen_wpb = 4; in.frozen_team = 1;
    return in;
}
static const size_t NTAB = 2 * 14 * 64;      // 1792

static void test_layout() {
    const FrozenPlanIn in = tiny();
    CHECK(frozen_row_doubles(in, true, false) == 35 && frozen_row_doubles(in, true, true) == 39);
    CHECK(frozen_row_doubles(in, false, false) == 5435 && frozen_row_doubles(in, false, true) == 5439);
    const size_t n = 7;
    for (const size_t B : {(size_t)1, (size_t)3, (size_t)7, (size_t)12})
        for (int form = 0; form < 4; ++form) {
            const bool lean = form & 1, src = form & 2;
            const size_t per_row = lean ? (src ? 39 : 35) : (src ? 5439 : 5435);
            const FrozenLayout L = frozen_layout(in, B, lean, src);
            CHECK(L.block_doubles == B * per_row);
            // every row position of every block that holds one of the n rows: its slots' places, block by block
            const size_t nblocks = (n + B - 1) / B;
            std::vector<std::vector<std::pair<size_t, size_t>>> iv(nblocks);
            for (size_t i = 0; i < nblocks * B; ++i)
                for (int slot = FROZEN_KV0; slot <= FROZEN_TCI; ++slot) {
                    if (slot == FROZEN_SRC && !src) continue;
                    if (slot >= FROZEN_FR && lean) continue;
                    const FrozenPlace p = frozen_place(L, i, slot);
                    CHECK(p.block == i / B);
                    const size_t len = slot <= FROZEN_KV2 ? 5 : slot == FROZEN_J ? 20 : slot == FROZEN_SRC ? 4 : slot <= FROZEN_FCI ? 8 : NTAB;
                    CHECK(p.offset + len <= B * per_row);        // inside its block
                    iv[p.block].push_back({p.offset, len});
                }
            // pairwise disjoint and without gaps: sorted, each starts where the one before ends, the last ends the block
            for (auto& v : iv) {
                std::sort(v.begin(), v.end());
                size_t end = 0;
                for (const auto& s : v) { CHECK(s.first == end); end = s.first + s.second; }
                CHECK(end == B * per_row);
            }
        }
    // B = cap: the slab, as the tables were carved out of it table by table ([cap][3][kv_len], [cap][5][np], [cap][nv] x 3,
    // [cap][ntab] x 3; lean with source planes: [cap][np] behind J)
    const size_t cap = 12;
    const FrozenLayout F = frozen_layout(in, cap, false, false), S = frozen_layout(in, cap, true, true);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) CHECK(frozen_place(F, i, FROZEN_KV0 + k).offset == (i * 3 + (size_t)k) * 5);
        const size_t J = cap * 15, fr = J + cap * 20, fcr = fr + cap * 8, fci = fcr + cap * 8, tr = fci + cap * 8, tcr = tr + cap * NTAB, tci = tcr + cap * NTAB;
        CHECK(frozen_place(F, i, FROZEN_J).offset == J + i * 20);
        CHECK(frozen_place(F, i, FROZEN_FR).offset == fr + i * 8 && frozen_place(F, i, FROZEN_FCR).offset == fcr + i * 8);
        CHECK(frozen_place(F, i, FROZEN_FCI).offset == fci + i * 8 && frozen_place(F, i, FROZEN_TR).offset == tr + i * NTAB);
        CHECK(frozen_place(F, i, FROZEN_TCR).offset == tcr + i * NTAB && frozen_place(F, i, FROZEN_TCI).offset == tci + i * NTAB);
        CHECK(frozen_place(F, i, FROZEN_J).block == 0);
        CHECK(frozen_place(S, i, FROZEN_J).offset == cap * 15 + i * 20 && frozen_place(S, i, FROZEN_SRC).offset == cap * 15 + cap * 20 + i * 4);
    }
    CHECK(F.oJ == 180 && F.ofr == 420 && F.ofcr == 516 && F.otr == 708 && F.otci == 708 + 2 * 12 * NTAB && F.oS == 0);
    CHECK(S.oS == 420 && S.ofr == 0 && S.otci == 0);      // (absent tables: 0)
}

static void test_admission_and_piece_rows() {
    // 0.85 / 1.02 x (1000 + 200) = 1000 bytes is the boundary
    CHECK(frozen_admit(999.9, 1000.0, 200.0) && !frozen_admit(1000.1, 1000.0, 200.0));
    CHECK(frozen_admit(999.9, 1200.0, 0.0) && !frozen_admit(1000.1, 1200.0, 0.0));
    FrozenPlanIn in = tiny();
    // 1 MiB: 1048576 / (8 x 35) = 3744.9, / (8 x 5435) = 24.1
    CHECK(frozen_piece_rows(in, true, false) == 3744 && frozen_piece_rows(in, false, false) == 24);
    in.frozen_cache_piece_mb = 1.0e-4;       // 104 bytes: less than a row
    CHECK(frozen_piece_rows(in, true, false) == 1);
    in.frozen_cache_piece_rows = 7;
    CHECK(frozen_piece_rows(in, true, false) == 7 && frozen_piece_rows(in, false, true) == 7);
}

static void test_keys() {
    CHECK(frozen_form_key(0, false, false, false) == 0);
    CHECK(frozen_form_key(0, true, false, false) == 0xC2B2AE3D27D4EB4Full);
    CHECK(frozen_form_key(0, true, true, false) == (0xC2B2AE3D27D4EB4Full ^ 0x165667B19E3779F9ull));
    CHECK(frozen_form_key(5, true, false, true) == (5 ^ 0xC2B2AE3D27D4EB4Full ^ 0x27D4EB2F165667C5ull));
    FrozenPlanIn in = tiny();
    in.frozen_err_check = 0;
    CHECK(frozen_key_full(in, 0, 0) == 0x9E3779B97F4A7C15ull);
    in.frozen_err_check = 1;
    CHECK(frozen_key_full(in, 6, 3) == (5 ^ (2 * 0x9E3779B97F4A7C15ull)));
    const double one_row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(frozen_sched_hash(one_row, 0) == 14695981039346656037ull);      // (FNV-1a: the offset basis for no bytes)
    CHECK(frozen_sched_hash(one_row, 1) != frozen_sched_hash(one_row, 0));
}

static void test_form() {
    FrozenPlanIn in = tiny();
    const int64_t n = 7;
    const uint64_t key = 0x1234;
    const double plenty = 1.0e6, scarce = 3.0e5;     // the full slab of 7 rows: 8 x 7 x 5435 = 304 360 bytes, x 1.02 = 310 447 > 0.85 x 300 000
    bool ruled = true;
    FrozenHeld none;
    in.frozen_cache_lean = 0; CHECK(frozen_form(in, n, key, none, 0, nullptr, &ruled) == 0 && !ruled);
    in.frozen_cache_lean = 1; CHECK(frozen_form(in, n, key, none, 0, nullptr, &ruled) == 1 && !ruled);
    in.frozen_cache_lean = 2;
    // refused by "frozen_cache_gb" (100 000 bytes): lean, and the device is not asked
    in.frozen_cache_max_gb = 1.0e-4;
    CHECK(frozen_form(in, n, key, none, 0, nullptr, &ruled) == 1 && !ruled);
    in.frozen_cache_max_gb = 1.0;
    // the 85 % rule: needs the free bytes, then decides
    CHECK(frozen_form(in, n, key, none, 0, nullptr, &ruled) == -1 && !ruled);
    CHECK(frozen_form(in, n, key, none, 0, &plenty, &ruled) == 0 && ruled);
    CHECK(frozen_form(in, n, key, none, 0, &scarce, &ruled) == 1 && ruled);
    // ... with what the cache holds counted as free: a lean slab of 24 rows, 8 x 24 x 35 = 6720 bytes -- 0.85 x (359 000 + 6720) = 310 862
    FrozenHeld lean_other;
    lean_other.lean = true; lean_other.blocks = 1; lean_other.block_rows = 24; lean_other.n = 5; lean_other.key = 99;
    const double just = 3.59e5;
    CHECK(frozen_form(in, n, key, none, 0, &just, &ruled) == 1 && frozen_form(in, n, key, lean_other, 0, &just, &ruled) == 0);
    // room in a held full cache: full, nobody asked
    FrozenHeld full_slab;
    full_slab.blocks = 1; full_slab.block_rows = 10;
    CHECK(frozen_form(in, n, key, full_slab, 0, nullptr, &ruled) == 0 && !ruled);
    full_slab.block_rows = 6;
    CHECK(frozen_form(in, n, key, full_slab, 0, nullptr, &ruled) == -1);
    in.frozen_cache_pieces = 1; in.frozen_cache_piece_rows = 3;      // 7 rows: 3 pieces of 3
    FrozenHeld full_pieces;
    full_pieces.pieces = true; full_pieces.blocks = 3; full_pieces.block_rows = 3;
    CHECK(frozen_form(in, n, key, full_pieces, 0, nullptr, &ruled) == 0 && !ruled);
    full_pieces.blocks = 2;
    CHECK(frozen_form(in, n, key, full_pieces, 0, nullptr, &ruled) == -1);
    full_slab.block_rows = 10;
    CHECK(frozen_form(in, n, key, full_slab, 0, nullptr, &ruled) == -1);       // (a slab is no room for pieces)
    in.frozen_cache_pieces = 0; in.frozen_cache_piece_rows = 0;
    // a held lean cache of this very schedule, chosen by the rule: stays lean, the device is not asked
    FrozenHeld lean_this;
    lean_this.lean = true; lean_this.blocks = 1; lean_this.block_rows = 24; lean_this.n = n; lean_this.key = key ^ FROZEN_LEAN_KEY;
    CHECK(frozen_form(in, n, key, lean_this, key, nullptr, &ruled) == 1 && !ruled);
    CHECK(frozen_form(in, n, key, lean_this, 0, nullptr, &ruled) == -1);
    CHECK(frozen_form(in, n + 1, key, lean_this, key, nullptr, &ruled) == -1);
    // what a thread is allocating stays what it is
    FrozenHeld busy;
    busy.alloc_state = 1; busy.alloc_lean = true;
    CHECK(frozen_form(in, n, key, busy, 0, nullptr, &ruled) == 1 && !ruled);
    busy.alloc_lean = false;
    CHECK(frozen_form(in, n, key, busy, 0, nullptr, &ruled) == 0);
    // a thresholded forced module and phosphorus: always lean
    for (const int mode : {0, 1, 2}) {
        FrozenPlanIn th = tiny();
        th.frozen_cache_lean = mode; th.kind = 2; th.sms_nrec = 3; th.sink_thres = 0.1;
        CHECK(frozen_form(th, n, key, none, 0, nullptr, &ruled) == 1 && !ruled);
        FrozenPlanIn ph = tiny();
        ph.frozen_cache_lean = mode; ph.kind = 1; ph.tc = 3;
        CHECK(frozen_form(ph, n, key, none, 0, nullptr, &ruled) == 1 && !ruled);
    }
    // the plan of a form
    in.frozen_cache_lean = 1;
    FrozenPlan pl = frozen_plan(in, n, key, true);
    CHECK(!pl.pieces && pl.lean && !pl.src && !pl.phos && pl.per_row == 35 && pl.B == 0 && pl.need == 0 && pl.bytes == 8.0 * 7 * 35 && pl.allowed);
    CHECK(pl.key == (key ^ FROZEN_LEAN_KEY));
    in.frozen_cache_pieces = 1; in.frozen_cache_piece_rows = 3;
    pl = frozen_plan(in, n, key, false);
    CHECK(pl.pieces && pl.B == 3 && pl.need == 3 && pl.bytes == 8.0 * 9 * 5435 && pl.key == key);
    in.frozen_cache_max_gb = 3.9e-4;         // 9 rows are 391 320 bytes
    CHECK(!frozen_plan(in, n, key, false).allowed);
    // one form at a time
    CHECK(!frozen_other_form(pl, none) && frozen_other_form(pl, full_slab) && frozen_other_form(pl, lean_this));
    full_pieces.blocks = 2;
    CHECK(!frozen_other_form(pl, full_pieces) && frozen_must_grow(pl, full_pieces, n));
    full_pieces.blocks = 3;
    CHECK(!frozen_must_grow(pl, full_pieces, n));
    full_pieces.block_rows = 4;
    CHECK(frozen_other_form(pl, full_pieces));
}

// rows of a schedule: t, t_new, h, n_iter, t_jac, h_lu, -, -
static std::vector<double> sched3(double t2 = 1.0, double last_iter = 1.0, double t_jac3 = 0.0) {
    return {0.0, 1.0, 1.0, 2.0, 0.0,    1.0, 0.0, 0.0,
            t2,  3.0, 2.0, 2.0, 0.0,    1.0, 0.0, 0.0,
            3.0, 4.0, 1.0, last_iter, t_jac3, 1.0, 0.0, 0.0};
}

static void test_eligible() {
    const FrozenPlanIn ok = tiny();
    CHECK(frozen_eligible(ok, sched3().data(), 3));
    CHECK(frozen_eligible(ok, sched3().data(), 1) && !frozen_eligible(ok, sched3().data(), 0));
    CHECK(!frozen_eligible(ok, sched3(1.5).data(), 3));          // the second row does not start where the first ends
    CHECK(!frozen_eligible(ok, sched3(1.0, 0.0).data(), 3));     // no Newton iteration on the last row
    {
        std::vector<double> s = sched3();
        s[3] = 0.0;                                              // ... or on one that hands over
        CHECK(!frozen_eligible(ok, s.data(), 3));
        s = sched3();
        s[8 + 2] = 1.5;                                          // a step not taken whole (t + h != t_new)
        CHECK(!frozen_eligible(ok, s.data(), 3));
    }
    FrozenPlanIn in = tiny();
    in.frozen_persistent = 0; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in = tiny(); in.hist_n = 1; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in = tiny(); in.norm_hook = true; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in = tiny(); in.factor_fp32 = 1; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in = tiny(); in.E = 7; in.frozen_persistent_max_e = 4; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.frozen_persistent_max_e = 8; CHECK(frozen_eligible(in, sched3().data(), 3));
    in.E = 9; in.frozen_persistent_max_e = 9; CHECK(!frozen_eligible(in, sched3().data(), 3));
    // the file-driven forced module at five levels per lane: with "frozen_forced" bit 1
    in = tiny(); in.kind = 2; in.E = 5;
    CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.frozen_forced = 1; CHECK(frozen_eligible(in, sched3().data(), 3));
    in.frozen_forced = 2; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.E = 4; in.frozen_forced = 0; CHECK(frozen_eligible(in, sched3().data(), 3));
    // a thresholded sink: with bit 2, and lean
    in = tiny(); in.kind = 2; in.sms_nrec = 2; in.sink_thres = 0.5;
    CHECK(frozen_thres(in) && !frozen_eligible(in, sched3().data(), 3));
    in.frozen_forced = 2; CHECK(!frozen_eligible(in, sched3().data(), 3));      // (no lean cache)
    in.frozen_cache_lean = 1; CHECK(frozen_eligible(in, sched3().data(), 3));
    in.frozen_forced = 1; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.E = 5; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.frozen_forced = 3; CHECK(frozen_eligible(in, sched3().data(), 3));
    in.sink_thres = 0.0; in.frozen_forced = 0; in.E = 2; CHECK(!frozen_thres(in) && frozen_eligible(in, sched3().data(), 3));
    // ... whose Jacobian time is a step start, the one before, or -- "jac_stage_state" -- a stage time of the row
    in = tiny(); in.kind = 2; in.sms_nrec = 2; in.sink_thres = 0.5; in.frozen_forced = 2; in.frozen_cache_lean = 2;
    const double stage = 3.0 + (1.0 * 0.6449489742783178);
    CHECK(frozen_eligible(in, sched3(1.0, 1.0, 3.0).data(), 3));
    CHECK(!frozen_eligible(in, sched3(1.0, 1.0, 3.5).data(), 3) && !frozen_eligible(in, sched3(1.0, 1.0, stage).data(), 3));
    in.jac_stage_state = 1;
    CHECK(!frozen_eligible(in, sched3(1.0, 1.0, 3.5).data(), 3) && frozen_eligible(in, sched3(1.0, 1.0, stage).data(), 3));
    in.t0 = -1.0;                                                // (a first row whose Jacobian time is neither t0, its start nor a stage time)
    {
        std::vector<double> s = sched3();
        s[4] = 0.25;
        CHECK(!frozen_eligible(in, s.data(), 3));
    }
    CHECK(frozen_eligible(tiny(), sched3(1.0, 1.0, 3.5).data(), 3));           // (linear sources: the Jacobian time is not looked at)
    // phosphorus: with "frozen_phosphorus", lean, from three levels per lane
    in = tiny(); in.kind = 1; in.tc = 3;
    CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.frozen_phosphorus = 1; in.frozen_cache_lean = 1;
    in.E = 2; CHECK(!frozen_phos(in) && !frozen_eligible(in, sched3().data(), 3));
    in.E = 3; CHECK(frozen_phos(in) && frozen_eligible(in, sched3().data(), 3));
    in.E = 8; CHECK(frozen_eligible(in, sched3().data(), 3));
    in.frozen_cache_lean = 0; CHECK(!frozen_eligible(in, sched3().data(), 3));
    in.frozen_cache_lean = 2; in.tc = 5; CHECK(!frozen_eligible(in, sched3().data(), 3));
}

static void test_growth() {
    FrozenPlanIn in = tiny();
    const int64_t n = 600;
    FrozenPlan pl = frozen_plan(in, n, 1, false);                // the full slab: 43 480 bytes a row
    FrozenHeld none;
    FrozenGrowth g = frozen_growth(in, pl, none, n, 1.0e12);
    CHECK(g.count == 1 && g.replace && g.block_rows == 600 + 100 + 16 && g.block_bytes == 716u * 43480u && !g.in_thread);
    // clamped by 0.9 x free: 0.9 x 31 420 000 / 43 480 = 650.4
    CHECK(frozen_growth(in, pl, none, n, 3.142e7).block_rows == 650);
    // ... plus what the old slab gives back: 100 rows more are 0.9 x 100 = 90 rows more room -- 740 > 716
    FrozenHeld old_slab;
    old_slab.blocks = 1; old_slab.block_rows = 100;
    CHECK(frozen_growth(in, pl, old_slab, n, 3.142e7).block_rows == 716);
    CHECK(frozen_growth(in, pl, none, n, 1000.0).block_rows == 600);          // never below n
    // pieces: those missing
    in.frozen_cache_pieces = 1; in.frozen_cache_piece_rows = 7;
    pl = frozen_plan(in, 33, 1, true);
    FrozenHeld two;
    two.pieces = true; two.lean = true; two.blocks = 2; two.block_rows = 7;
    g = frozen_growth(in, pl, two, 33, 0.0);
    CHECK(pl.need == 5 && g.count == 3 && !g.replace && g.block_rows == 7 && g.block_bytes == 8u * 7u * 35u && !g.in_thread);
    // the thread: above 8e9 bytes, and only with "frozen_alloc_async".  Rows of 8 x 2^20 doubles = 67 108 864 bytes
    FrozenPlanIn big = tiny();
    big.np = big.kv_len = (size_t)1 << 20;
    big.frozen_cache_max_gb = 1000.0;
    pl = frozen_plan(big, n, 1, true);
    CHECK(pl.per_row == (size_t)8 << 20);
    CHECK(frozen_growth(big, pl, none, n, 1.0e15).in_thread);                 // 716 rows: 48 GB
    CHECK(!frozen_growth(big, pl, none, 50, 1.0e15).in_thread);               // 74 rows: 5 GB
    big.frozen_alloc_async = 0;
    CHECK(!frozen_growth(big, pl, none, n, 1.0e15).in_thread);
    big.frozen_alloc_async = 1;
    big.frozen_cache_pieces = 1; big.frozen_cache_piece_rows = 10;            // pieces of 671 088 640 bytes: 12 are 8.05e9, 11 are 7.38e9
    CHECK(frozen_growth(big, frozen_plan(big, 120, 1, true), none, 120, 0.0).in_thread);
    CHECK(!frozen_growth(big, frozen_plan(big, 110, 1, true), none, 110, 0.0).in_thread);
    // "frozen_cache_after"
    in.frozen_cache_after = 2; CHECK(frozen_years_before_build(in, 1.0) == 2 && frozen_years_before_build(in, 9.0e9) == 2);
    in.frozen_cache_after = -1; CHECK(frozen_years_before_build(in, 7.0e9) == 0 && frozen_years_before_build(in, 9.0e9) == 3);
}

static int lds_bits(int E, int tc, int ny, int coef_lds, bool pieces, int by_column_opt = 1, int* by_column = nullptr) {
    FrozenPlanIn in = tiny();
    in.E = E; in.tc = tc; in.ny = ny; in.ncol = tc * ny; in.frozen_coef_lds = coef_lds; in.frozen_by_column = by_column_opt;
    int bits = -1, bc = -1;
    frozen_lds_shape(in, false, false, pieces, 256, &bits, &bc);
    if (by_column) *by_column = bc;
    return bits;
}

static void test_lds() {
    // in units of 64 doubles (512 bytes; a compute unit has 320): by column a workgroup takes (7 E + 1) coefficients + 5 E step block
    // + per wave 3 E (W) + E (pivots) + E (Y)
    CHECK(frozen_lds_doubles(7, 63, true, 3) == 64u * (50 + 35 + 3 * (21 + 7 + 7)));
    CHECK(frozen_lds_doubles(7, 3, true, 3) == 64u * (50 + 3 * 21) && frozen_lds_doubles(5, 0, true, 3) == 0);
    CHECK(frozen_lds_doubles(4, 3, false, 4) == 64u * 4 * (29 + 12) && frozen_lds_doubles(4, 1, false, 4) == 64u * 4 * 29);
    // 416 ypos columns on 256 compute units: two workgroups on one.  E = 5: 86 / 136 units a workgroup -- fits twice
    CHECK(lds_bits(5, 1, 416, 63, false) == 63 && lds_bits(5, 3, 416, 63, false) == 63);
    // E = 6: 103, fits; three tracers 163 x 2 = 326: Y goes (145 x 2 = 290) -- the stage values stay, except on pieces
    CHECK(lds_bits(6, 1, 416, 63, false) == 63 && lds_bits(6, 3, 416, 63, false) == 47 && lds_bits(6, 3, 416, 63, true) == 15);
    // E = 7: 120, fits; three tracers 190 x 2: Y goes (169 x 2 = 338), the pivots go (148 x 2 = 296) -- and with a part of 15
    // missing both own-state bits
    CHECK(lds_bits(7, 1, 416, 63, false) == 63 && lds_bits(7, 3, 416, 63, false) == 7);
    // E = 8 has no own state: 129 fits; three tracers 193 x 2: (Y is not there,) pivots (169 x 2), step block (129 x 2 = 258)
    CHECK(lds_bits(8, 1, 416, 63, false) == 15 && lds_bits(8, 3, 416, 63, false) == 3);
    // 26 ypos columns: one workgroup on a compute unit, everything fits
    for (const int tc : {1, 3}) {
        CHECK(lds_bits(5, tc, 26, 63, false) == 63 && lds_bits(6, tc, 26, 63, false) == 63 && lds_bits(7, tc, 26, 63, false) == 63);
        CHECK(lds_bits(8, tc, 26, 63, false) == 15);
    }
    // the own state only on top of all of 15; bit 32 without 16 not on pieces
    CHECK(lds_bits(5, 1, 416, 55, false) == 7 && lds_bits(5, 1, 416, 47, false) == 47 && lds_bits(5, 1, 416, 47, true) == 15);
    // not by column: coefficients and W only; below three levels per lane nothing
    int bc = -1;
    CHECK(lds_bits(5, 1, 416, 63, false, 0, &bc) == 3 && bc == 0);
    CHECK(lds_bits(4, 1, 416, 63, false, 1, &bc) == 3 && bc == 0);
    CHECK(lds_bits(4, 1, 416, 63, false, 2, &bc) == 15 && bc == 1);
    CHECK(lds_bits(2, 1, 416, 63, false, 2, &bc) == 0 && bc == 0);
    // phosphorus: by column whatever the options say, no own state
    FrozenPlanIn ph = tiny();
    ph.E = 5; ph.kind = 1; ph.tc = 3; ph.ny = 26; ph.ncol = 78; ph.frozen_by_column = 0; ph.frozen_coef_lds = 0;
    int bits = -1;
    frozen_lds_shape(ph, true, true, false, 256, &bits, &bc);
    CHECK(bits == 0 && bc == 1);
    ph.frozen_coef_lds = 63;
    frozen_lds_shape(ph, true, true, false, 256, &bits, &bc);
    CHECK(bits == 15 && bc == 1);     // (36 + 25 + 3 x 20 = 121 units: fits)
}

int main() {
    test_layout();
    test_admission_and_piece_rows();
    test_keys();
    test_form();
    test_eligible();
    test_growth();
    test_lds();
    if (failures == 0) std::printf("frozen plan ok\n");
    return failures == 0 ? 0 : 1;
}
