// Option "frozen_dedicated" in the arithmetic of the one-launch frozen year (csrc/nk2d_frozen_plan.h): which years the entry with the
// default year's body alone (k_frozen_persistent_d) takes.  Under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU:
// `make -C newton-krylov_ooc_amd/csrc asan-host` (tests/test_frozen_dedicated_host.py runs it).  Known answers only, worked out by
// hand from the rule the header states: option 1 or 2; a wave per column on the full cache; five to seven levels per lane; the
// linear-source kinds 0 and 2; all six LDS bits; "frozen_early", the stage-value exchange and the VALU moves in effect; and not the
// piece flavours <7, 0> (no exchange body) and <6, 0> (no VALU body) of k_frozen_persistent.
#include <cstdio>

#include "nk2d_frozen_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the year of the benchmark: seven levels per lane, kind 0, the slab, everything on
static int bench(int option) { return frozen_dedicated(option, 7, 0, false, false, false, 63, 1, 1, 1); }

static void test_option_values() {
    CHECK(bench(0) == 0);
    CHECK(bench(1) == 1);
    CHECK(bench(2) == 2);
    // (the library refuses other values when the option is set; the rule reads them as 0)
    CHECK(bench(3) == 0 && bench(-1) == 0);
}

static void test_instantiations() {
    // the set, written out: (E, kind, pieces) -> has an instantiation
    struct Row { int E, kind, pieces; bool has; };
    const Row rows[] = {
        {5, 0, 0, true}, {5, 0, 1, true}, {5, 2, 0, true}, {5, 2, 1, true},
        {6, 0, 0, true}, {6, 0, 1, false}, {6, 2, 0, true}, {6, 2, 1, true},
        {7, 0, 0, true}, {7, 0, 1, false}, {7, 2, 0, true}, {7, 2, 1, true},
        {4, 0, 0, false}, {8, 0, 0, false}, {3, 2, 1, false}, {1, 0, 0, false},
        {5, 1, 0, false}, {6, 1, 1, false}, {7, 1, 0, false},
    };
    int has = 0;
    for (const Row& r : rows) {
        CHECK((NK2D_FROZEN_DEDICATED(r.E, r.kind, r.pieces) != 0) == r.has);
        for (const int option : {1, 2})
            CHECK(frozen_dedicated(option, r.E, r.kind, false, r.pieces != 0, false, 63, 1, 1, 1) == (r.has ? option : 0));
        CHECK(frozen_dedicated(0, r.E, r.kind, false, r.pieces != 0, false, 63, 1, 1, 1) == 0);
        has += r.has ? 1 : 0;
    }
    CHECK(has == 10);
    // every instantiation of the set is one k_frozen_persistent has the VALU body for
    for (int E = 1; E <= 8; ++E)
        for (const int kind : {0, 1, 2})
            for (const int pieces : {0, 1})
                CHECK((NK2D_FROZEN_DEDICATED(E, kind, pieces) != 0) == (NK2D_FROZEN_XLANE(E, kind, 0, pieces, 0) != 0));
}

static void test_year_must_run_the_body() {
    // a team year, a lean cache: never
    CHECK(frozen_dedicated(1, 7, 0, true, false, false, 63, 1, 1, 1) == 0);
    CHECK(frozen_dedicated(2, 7, 0, false, false, true, 63, 1, 1, 1) == 0);
    CHECK(frozen_dedicated(1, 5, 2, false, true, true, 63, 1, 1, 1) == 0);
    // any part of the column not in LDS, or the own state not whole: another body
    for (const int bits : {0, 1, 3, 7, 15, 31, 47, 62})
        for (const int option : {1, 2}) CHECK(frozen_dedicated(option, 7, 0, false, false, false, bits, 1, 1, 1) == 0);
    // "frozen_early" 0 (CL 959 is compiled with the deferred partial), the exchange 0 (CL 191), the VALU moves 0 (CL 447)
    CHECK(frozen_dedicated(1, 7, 0, false, false, false, 63, 0, 1, 1) == 0);
    CHECK(frozen_dedicated(1, 7, 0, false, false, false, 63, 1, 0, 0) == 0);
    CHECK(frozen_dedicated(1, 7, 0, false, false, false, 63, 1, 1, 0) == 0);
    CHECK(frozen_dedicated(2, 6, 2, false, true, false, 63, 1, 1, 0) == 0);
    CHECK(frozen_dedicated(2, 6, 2, false, true, false, 63, 1, 1, 1) == 2);
}

static void test_with_the_lds_shape() {
    // the bits as frozen_lds_shape() grants them.  416 x 416 iage (two tracers) on 256 compute units: two workgroups of two waves on a
    // compute unit.  Doubles: coefficients (7 * 7 + 1) * 64 = 3200, step block 5 * 7 * 64 = 2240, per wave W 1344 + pivots 448 + Y 448
    // = 2240: 9920 doubles = 79 360 bytes, twice that 158 720 <= 163 840: all six bits stay
    FrozenPlanIn in = {};
    in.E = 7; in.kind = 0; in.tc = 2; in.ny = 416; in.ncol = 832;
    in.frozen_coef_lds = 63; in.frozen_by_column = 1; in.frozen_wpb = 4; in.frozen_team = 1;
    int bits = -1, by_col = -1;
    frozen_lds_shape(in, false, false, false, 256, &bits, &by_col);
    CHECK(frozen_lds_doubles(7, 63, true, 2) == 9920);
    CHECK(bits == 63 && by_col == 1);
    CHECK(frozen_dedicated(1, in.E, in.kind, false, false, false, bits, 1, 1, 1) == 1);
    // the lean cache has no own state: 15, the entry is not taken
    frozen_lds_shape(in, false, true, false, 256, &bits, &by_col);
    CHECK(bits == 15);
    CHECK(frozen_dedicated(1, in.E, in.kind, false, false, true, bits, 0, 0, 0) == 0);
    // eight levels per lane: no own state either
    in.E = 8;
    frozen_lds_shape(in, false, false, false, 256, &bits, &by_col);
    CHECK((bits & 48) == 0);
    CHECK(frozen_dedicated(2, in.E, in.kind, false, false, false, bits, 0, 0, 0) == 0);
    // option "frozen_coef_lds" 15: the bodies from before the own state
    in.E = 7; in.frozen_coef_lds = 15;
    frozen_lds_shape(in, false, false, false, 256, &bits, &by_col);
    CHECK(bits == 15 && frozen_dedicated(1, 7, 0, false, false, false, bits, 0, 0, 0) == 0);
}

int main() {
    test_option_values();
    test_instantiations();
    test_year_must_run_the_body();
    test_with_the_lds_shape();
    if (failures == 0) std::printf("frozen plan dedicated ok\n");
    return failures == 0 ? 0 : 1;
}
