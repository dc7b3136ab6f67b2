// Option "frozen_phosphorus_shallow" in the arithmetic of the schedule cache of the one-launch frozen year (csrc/nk2d_frozen_plan.h):
// the phosphorus module at one and two levels per lane.  Under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU:
// `make -C newton-krylov_ooc_amd/csrc asan-host` (tests/test_frozen_phosphorus_shallow_host.py runs it).  Known answers only,
// worked out by hand from the rules the header states.
#include <cstdio>
#include <vector>

#include "nk2d_frozen_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// a phosphorus context of six ypos columns at E levels per lane: three tracers, planes of 6 x 64 E doubles
static FrozenPlanIn phos(int E) {
    FrozenPlanIn in = {};
    in.E = E; in.kind = 1; in.tc = 3; in.ny = 6; in.ncol = 18;
    in.np = (size_t)6 * 64 * E; in.kv_len = in.np; in.nv = 3 * in.np;
    in.frozen_persistent = 1; in.frozen_persistent_max_e = 8;
    in.frozen_phosphorus = 1; in.frozen_cache_lean = 1;
    in.frozen_cache_piece_mb = 1024.0; in.frozen_cache_max_gb = 128.0;
    in.frozen_coef_lds = 63; in.frozen_by_column = 1; in.frozen_wpb = 4; in.frozen_team = 1;
    return in;
}

// three rows that hand over; the Jacobian is evaluated at every step start (t, t_new, h, n_iter, t_jac, h_lu, -, -)
static std::vector<double> sched3() {
    return {0.0, 1.0, 1.0, 2.0, 0.0, 1.0, 0.0, 0.0,
            1.0, 3.0, 2.0, 2.0, 1.0, 2.0, 0.0, 0.0,
            3.0, 4.0, 1.0, 1.0, 3.0, 1.0, 0.0, 0.0};
}

static void test_routing() {
    const std::vector<double> s = sched3();
    // a plan input that names nothing: the field is 0, and two levels per lane stay out
    FrozenPlanIn zero = {};
    CHECK(zero.frozen_phosphorus_shallow == 0);
    for (const int E : {1, 2, 3}) {
        for (const int shallow : {0, 1}) {
            FrozenPlanIn in = phos(E);
            in.frozen_phosphorus_shallow = shallow;
            const bool want = E >= 3 || shallow == 1;
            CHECK(frozen_phos(in) == want);
            CHECK(frozen_eligible(in, s.data(), 3) == want);
            // values 2 and 3 of "frozen_phosphorus", and mode 2 of the lean cache: the same answer
            for (const int value : {2, 3}) { in.frozen_phosphorus = value; CHECK(frozen_phos(in) == want); }
            in.frozen_phosphorus = 1; in.frozen_cache_lean = 2;
            CHECK(frozen_phos(in) == want && frozen_eligible(in, s.data(), 3) == want);
            // without the lean cache, without "frozen_phosphorus", with more tracers than a workgroup has waves: never
            in.frozen_cache_lean = 0;
            CHECK(!frozen_phos(in) && !frozen_eligible(in, s.data(), 3));
            in.frozen_cache_lean = 1; in.frozen_phosphorus = 0;
            CHECK(!frozen_phos(in) && !frozen_eligible(in, s.data(), 3));
            in.frozen_phosphorus = 1; in.tc = 5;
            CHECK(!frozen_phos(in) && !frozen_eligible(in, s.data(), 3));
            // what keeps any one-launch year out keeps this one out
            in.tc = 3;
            in.factor_fp32 = 1; CHECK(!frozen_eligible(in, s.data(), 3)); in.factor_fp32 = 0;
            in.hist_n = 1; CHECK(!frozen_eligible(in, s.data(), 3)); in.hist_n = 0;
            in.norm_hook = true; CHECK(!frozen_eligible(in, s.data(), 3)); in.norm_hook = false;
            CHECK(frozen_eligible(in, s.data(), 3) == want);
        }
    }
    // the Jacobian-time check holds here as at any depth: a Jacobian time that is neither the row's start nor the one before
    FrozenPlanIn in = phos(2);
    in.frozen_phosphorus_shallow = 1;
    std::vector<double> bad = sched3();
    bad[2 * 8 + 4] = 3.5;
    CHECK(!frozen_eligible(in, bad.data(), 3));
    bad[2 * 8 + 4] = 1.0;                    // (reuses the row before's)
    CHECK(frozen_eligible(in, bad.data(), 3));
    // other modules do not read the field
    for (const int kind : {0, 2}) {
        FrozenPlanIn o = phos(2);
        o.kind = kind; o.tc = 1; o.ncol = 6; o.nv = o.np;
        const bool before = frozen_eligible(o, s.data(), 3);
        o.frozen_phosphorus_shallow = 1;
        CHECK(!frozen_phos(o) && frozen_eligible(o, s.data(), 3) == before && before);
    }
}

static void test_lds_shape() {
    // nothing of the year in LDS below three levels per lane, and the workgroup is the ypos column -- whatever the options say
    for (const int E : {1, 2})
        for (const int coef : {0, 1, 3, 7, 15, 63})
            for (const int by_col : {0, 1, 2})
                for (const int team : {0, 1})
                    for (const int pieces : {0, 1})
                        for (const int ny : {2, 6, 416}) {
                            FrozenPlanIn in = phos(E);
                            in.frozen_phosphorus_shallow = 1;
                            in.frozen_coef_lds = coef; in.frozen_by_column = by_col; in.frozen_team = team;
                            in.ny = ny; in.ncol = 3 * ny;
                            int bits = -1, bc = -1;
                            frozen_lds_shape(in, true, true, pieces != 0, 256, &bits, &bc);
                            CHECK(bits == 0 && bc == 1);
                        }
    CHECK(frozen_lds_doubles(1, 0, true, 3) == 0 && frozen_lds_doubles(2, 0, true, 3) == 0);
}

static void test_rows_and_key() {
    for (const int E : {1, 2}) {
        FrozenPlanIn in = phos(E);
        in.frozen_phosphorus_shallow = 1;
        const size_t plane = (size_t)6 * 64 * E;             // 384, 768
        CHECK(frozen_row_doubles(in, true, false) == 3 * plane + 5 * plane);
        bool ruled = true;
        FrozenHeld none;
        for (const int mode : {1, 2}) {
            in.frozen_cache_lean = mode;
            CHECK(frozen_form(in, 7, 0x1234, none, 0, nullptr, &ruled) == 1 && !ruled);      // always lean, the device is not asked
        }
        in.frozen_cache_lean = 1;
        FrozenPlan pl = frozen_plan(in, 7, 0x1234, true);
        CHECK(pl.lean && pl.phos && !pl.src && !pl.pieces && pl.per_row == 8 * plane);
        CHECK(pl.bytes == 8.0 * 7.0 * 8.0 * (double)plane && pl.allowed);
        // the form key is the phosphorus one
        CHECK(pl.key == (0x1234ull ^ 0xC2B2AE3D27D4EB4Full ^ 0x27D4EB2F165667C5ull));
        CHECK(pl.key == frozen_form_key(0x1234, true, false, true));
        // ... and the full key does not read the option
        FrozenPlanIn off = in;
        off.frozen_phosphorus_shallow = 0;
        CHECK(frozen_key_full(in, 6, 3) == frozen_key_full(off, 6, 3));
        // pieces of 7 rows: 23 rows are 4 pieces, 28 rows of 8 planes
        in.frozen_cache_pieces = 1; in.frozen_cache_piece_rows = 7;
        pl = frozen_plan(in, 23, 0x1234, true);
        CHECK(pl.pieces && pl.B == 7 && pl.need == 4 && pl.bytes == 8.0 * 28.0 * 8.0 * (double)plane);
        const FrozenLayout L = frozen_layout(in, 7, true, false);
        CHECK(L.block_doubles == 7 * 8 * plane && L.oJ == 7 * 3 * plane && L.oS == 0 && L.ofr == 0);
        CHECK(frozen_place(L, 9, FROZEN_J).block == 1 && frozen_place(L, 9, FROZEN_J).offset == L.oJ + 2 * 5 * plane);
    }
}

int main() {
    test_routing();
    test_lds_shape();
    test_rows_and_key();
    if (failures == 0) std::printf("frozen plan shallow ok\n");
    return failures == 0 ? 0 : 1;
}
