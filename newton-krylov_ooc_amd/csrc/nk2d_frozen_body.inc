// nk2d_frozen_body.inc -- the body of the one-launch frozen year's kernel (nk2d_frozen.hip): included inside k_frozen_persistent and
// k_frozen_persistent_w2, which name E, KIND, TEAM, PIECES, LEAN and the arguments P and A.  Not a header: no guard, no declarations.
// The includer also names FZ_ONLY.  0: the text as it always was -- every body of the ladder, picked at run time from A.coef_lds.
// 959 (k_frozen_persistent_d, nk2d_frozen_d.hip): the body of the default year alone, CL 959, and what the host guarantees for
// that body (frozen_dedicated(), nk2d_frozen_plan.h) as compile-time truth: by column; W, the step block, the pivots and Y in
// LDS; the whole own state; "frozen_early", the stage-value exchange and the VALU moves on.  Bit 11 of A.coef_lds then picks the
// hand-over's poll.  Every `#if FZ_ONLY` below leaves the 0 text token for token what it was.
#if FZ_ONLY
    static_assert(FZ_ONLY == 959 && !TEAM && !LEAN && NK2D_FROZEN_OWN(E, KIND, TEAM, LEAN), "the dedicated entry: the one body of the default year");
#endif
    constexpr int XCD = 0, NB = 1;      // (rounds 2 - 3 also had all workgroups on one XCD and a grid barrier between the phases)
    __shared__ int lds_ok;
    __shared__ double team_lds[TEAM ? sizeof(TeamLds<E, 3>) / sizeof(double) : 1];
    constexpr int MPX = XCD ? 2 : 1;
    const int lane = threadIdx.x & 63;
    int wg = (int)blockIdx.x;
    const int tw = uni_i((int)(threadIdx.x >> 6));                      // TEAM: the wave's place in its team
    // the column of this wave.  A team: the workgroup's.  A wave per column: adjacent columns of one tracer to a workgroup, or
    // -- `by_column` -- the workgroup is ONE ypos column and its waves that column's tracers (what is the same for every tracer
    // of a ypos column is then shared through LDS)
#if FZ_ONLY
    (void)team_lds;
    constexpr bool by_col = true;
#else
    const bool by_col = !TEAM && !XCD && NB != 0 && A.by_column != 0;
#endif
    const int wave = TEAM ? uni_i(wg) : (by_col ? uni_i(tw * P.ny + wg) : uni_i(wg * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6)));
    const bool col_wave = wave < P.ncol && (!by_col || (tw < P.tc && wg < P.ny));
    // NB: neighbour-to-neighbour hand-over instead of the grid barrier.  The unit is the workgroup: one column (teams), or
    // the columns of its waves -- then the workgroup to the left matters if its first column has a left neighbour, the one to
    // the right if its last column has a right neighbour (a tracer boundary inside the workgroup needs nothing)
    int nb_left, nb_right;
    if constexpr (TEAM) {
        const int nb_j = wave % P.ny;
        nb_left = (nb_j > 0) ? wg - 1 : -1;
        nb_right = (nb_j < P.ny - 1) ? wg + 1 : -1;
    } else if (by_col) {
        nb_left = (wg > 0) ? wg - 1 : -1;
        nb_right = (wg < P.ny - 1) ? wg + 1 : -1;
    } else {
        const int wpb = (int)(blockDim.x >> 6);
        const int c0 = wg * wpb, cl = min(c0 + wpb - 1, P.ncol - 1);
        nb_left = (c0 % P.ny > 0) ? wg - 1 : -1;
        nb_right = (cl % P.ny < P.ny - 1) ? wg + 1 : -1;
    }
    NeighbourSync nbs{(unsigned*)((char*)A.arrive + 8192), A.abort_flag, wg, nb_left, nb_right, 0u, &lds_ok, A.spin_ticks, A.fences};
#ifdef NK2D_FROZEN_CLOCKS
    const long long ck_begin = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    const size_t nv = A.C.nv;
    int swapY = 0, swapZ = 0, status = 0, done = 0;
    int pc_p = 0, pc_r = 0;     // PIECES: row i is row pc_r of piece pc_p (i = pc_p rows + pc_r, kept by counting: no division)
    (void)pc_p; (void)pc_r;
#define FZ_Y (swapY ? A.YOLD : A.Y)
#define FZ_YOLD (swapY ? A.Y : A.YOLD)
#define FZ_Z (swapZ ? A.ZN : A.Z)
#define FZ_ZN (swapZ ? A.Z : A.ZN)
#define FZ_SYNC() \
    if (!nbs.sync()) { status = 1; goto finish; }
    // behind a phase whose body does not carry the stage values: nothing of OwnState::z is kept through the next one's solves
#define FZ_OWN_DEAD() \
    if constexpr (OWN) { \
        _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_) { \
            _Pragma("unroll") for (int e_ = 0; e_ < E; ++e_) own.z[r_][e_] = 0.0; \
        } \
    }
    // a wave per column, three and more levels per lane (option "frozen_coef_lds"): the static coefficients of the wave's column
    // in LDS for the whole year (dynamic shared memory of the launch: NK2D_COEF_LDS_DOUBLES(E) doubles per wave)
    constexpr bool COEF_LDS = NB != 0 && !TEAM && !XCD && E >= 3;
    // Layout of the dynamic shared memory.  Adjacent columns: per wave [coefficients][W].  By column: [coefficients of the ypos
    // column][step block: 3 mixing columns, JL, JU][per wave: W][per wave: pivots of the real system][per wave: own Y] (each part
    // present where its bit of A.coef_lds is set; frozen_lds_doubles() on the host computes the same)
    extern __shared__ double dyn_lds[];
#if FZ_ONLY
    constexpr bool w_in_lds = true, step_in_lds = true, piv_in_lds = true;
#else
    const bool w_in_lds = COEF_LDS && (A.coef_lds & 2) != 0;
    const bool step_in_lds = COEF_LDS && by_col && (A.coef_lds & 4) != 0;
    const bool piv_in_lds = COEF_LDS && by_col && (A.coef_lds & 8) != 0;
#endif
    // the column's own state from phase to phase (OwnState; bits 16, 32 of A.coef_lds -- the host sets them only on top of the
    // full by-column set 15): Y in LDS, the stage values in registers.  Compiled in where the registers hold it; the piece
    // flavour has the stage values only together with Y (with all three bodies <7, 0, 0, 1, 0> spills a register)
    constexpr bool OWN = COEF_LDS && NK2D_FROZEN_OWN(E, KIND, TEAM, LEAN);
#if FZ_ONLY
    constexpr int own_bits = 48;
#else
    const int own_bits = OWN && by_col ? (A.coef_lds & 48) : 0;
#endif
    (void)own_bits;
    const int nwv = (int)(blockDim.x >> 6);
    double* my_coef;
    double* my_w;
    double* step_lds = nullptr;
    double* my_piv = nullptr;
    double* my_y = nullptr;
    if (by_col) {
        double* p = dyn_lds;
        my_coef = p; p += NK2D_COEF_LDS_DOUBLES(E);
        step_lds = p; p += step_in_lds ? 5 * E * 64 : 0;
        my_w = p + (size_t)tw * (3 * E * 64); p += w_in_lds ? (size_t)nwv * 3 * E * 64 : 0;
        my_piv = p + (size_t)tw * (E * 64); p += piv_in_lds ? (size_t)nwv * E * 64 : 0;
        my_y = p + (size_t)tw * (E * 64);
    } else {
        my_coef = dyn_lds + (size_t)(threadIdx.x >> 6) * (NK2D_COEF_LDS_DOUBLES(E) + (w_in_lds ? 3 * E * 64 : 0));
        my_w = my_coef + NK2D_COEF_LDS_DOUBLES(E);
    }
    const LdsSrc L = {my_coef, my_w, step_lds, my_piv, my_y};
    (void)L;
    OwnState<OWN ? E : 1> own;
    own.valid = 0;      // (the year's first phase reads the state the host put there and the zeros stored below)
    if constexpr (OWN) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int e = 0; e < E; ++e) own.z[r][e] = 0.0;
        }
    }
    if constexpr (COEF_LDS) {
        if (A.coef_lds && col_wave && (!by_col || tw == 0)) {
            ColCoef<E> cf;
            load_coef<E>(P, wave % P.ny, lane, cf);
            store_coef_lds<E>(my_coef, lane, cf);
        }
        if (by_col && A.coef_lds) __syncthreads();      // (the other tracers' waves read what wave 0 stored)
    }
    int lds_step = -1;      // the step whose constants the step block / the pivots hold
    (void)lds_step;
    // option "frozen_early" (bit 8 of A.coef_lds, set by the host only where the year carries the whole own state, CL 63): the wave
    // forms the norm partial of an update part behind that part's stores and stores it behind the hand-over's flag (LateNorm)
#if FZ_ONLY
    LateNorm late = {0.0, nullptr, 1, 0};
#else
    LateNorm late = {0.0, nullptr, (OWN && by_col && own_bits == 48) ? uni_i(NK2D_FROZEN_EARLY_OF(A.coef_lds)) : 0, 0};
#endif
    (void)late;
    // option "frozen_stage_exchange" (bit 9 of A.coef_lds, under the same rule): the neighbours exchange the stage values U_i = Y + Z_i,
    // not Z_i and Y (StageXchg).  U and UN lie behind the synchronisation block; their parity is Z's and ZN's (swapZ)
#if FZ_ONLY
    constexpr bool XCHG = OWN;
    constexpr int xchg = 1;
#else
    constexpr bool XCHG = OWN && NK2D_FROZEN_XCHG(E, KIND, TEAM, PIECES, LEAN);     // (compiled in where it costs no spilled register)
    const int xchg = (XCHG && by_col && own_bits == 48) ? uni_i(NK2D_FROZEN_XCHG_OF(A.coef_lds)) : 0;
#endif
    double* const xu0 = XCHG ? (double*)((char*)A.arrive + yr_xchg_offset(P.ncol)) : nullptr;
    (void)xchg; (void)xu0;
    // option "frozen_xlane" (bit 10 of A.coef_lds, set by the host only on top of bit 9): the body whose cross-lane moves go through the VALU
#if FZ_ONLY
    // the hand-over's poll (bit 11 of A.coef_lds, option "frozen_dedicated" 2): NeighbourSync::wait_one_load() instead of wait()
    const int poll_one = uni_i((A.coef_lds >> 11) & 1);
#else
    constexpr bool XLANE = XCHG && NK2D_FROZEN_XLANE(E, KIND, TEAM, PIECES, LEAN);
    const int xlane = (XLANE && xchg) ? uni_i(NK2D_FROZEN_XLANE_OF(A.coef_lds)) : 0;
    (void)xlane;
#endif
#define FZ_U (swapZ ? xu0 + 3 * nv : xu0)
#define FZ_UN (swapZ ? xu0 : xu0 + 3 * nv)
    // first attempt of the year: Z0 = 0, W0 = 0 (radau.py:445-446)
    if (col_wave && (!TEAM || tw == 0)) {
        double zero[E];
#pragma unroll
        for (int e = 0; e < E; ++e) zero[e] = 0.0;
        if constexpr (XCHG) {
            if (xchg) {     // U0 = Y + Z0, by the addition itself (a -0.0 of Y comes out as the stage part's own sum gave it)
                double y0[E];
                load_col<E, MPX>(FZ_Y, wave, lane, y0);
#pragma unroll
                for (int e = 0; e < E; ++e) y0[e] = y0[e] + zero[e];
#pragma unroll
                for (int i = 0; i < 3; ++i) store_col<E, 1>(FZ_U + i * nv, wave, lane, y0);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            store_col<E, MPX>(FZ_Z + i * nv, wave, lane, zero);
            store_col<E, (TEAM ? MPX : 0)>(A.W + i * nv, wave, lane, zero);
            if constexpr (COEF_LDS) {
                if (w_in_lds) w_lds_put<E>(my_w, i, lane, zero);
            }
        }
    }
    FZ_SYNC()
    for (int i = 0; i < A.n; ++i) {
        const FrozenRow R = A.rows[i];
        const int n_iter = uni_i(R.n_iter), m = uni_i(R.m);
        const bool last_row = i == A.n - 1;
        // PIECES: the row's tables -- the piece's base (the same for every lane of every wave: one load, the value in scalar
        // registers) + fixed offsets + r stride; the slab flavour forms base + i stride where it uses them, as it always did
        RowTabs T = {};
        const double* kv_prev = nullptr;    // the mixing plane at the step start = the last stage plane of row i - 1
        (void)T; (void)kv_prev;
        if constexpr (PIECES) {
            double* const base = uni_p(A.T.base[pc_p]);
            T = piece_row_tabs(A.C, A.T, base, pc_r);
            if (i > 0 && uni_i(R.err) != 0) {
                // (row i - 1 may be the last row of the piece before: resolved on its own, on the few rows that carry an estimate)
                const double* pb = pc_r > 0 ? base : uni_p(A.T.base[pc_p - 1]);
                const int pr = pc_r > 0 ? pc_r - 1 : A.T.rows - 1;
                kv_prev = pb + ((size_t)pr * 3 + 2) * A.C.kv_len;
            }
            if (++pc_r == A.T.rows) { pc_r = 0; ++pc_p; }
        }
        const double* kvb = PIECES ? T.KV : A.C.KV + (size_t)i * 3 * A.C.kv_len;
        const double* J = PIECES ? T.J : A.C.J + (size_t)i * 5 * A.C.np;
        if constexpr (KIND == 1 && LEAN) {
            // phosphorus (option "frozen_phosphorus"): UPR = d uptake / d po4 of the workgroup's ypos column, at the rows where the launch
            // path evaluates the Jacobian anew, from tracer 0 of the state at the step start (the workgroup's own y_new of the row
            // before, or the year's input) -- jac_core's expressions, into the plane P.UPR names (the cache's own).  EVERY wave of
            // the workgroup forms the column for itself, with the accessor its stage tendencies load another tracer's state with:
            // the same values to the same places, each wave waits for its own stores and reads back no other wave's
            if (A.upr_on != 0 && uni_i(R.upr) != 0 && col_wave) {
                phos_upr_col<E, 0>(P, FZ_Y, const_cast<double*>(P.UPR), wave % P.ny, lane);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        if constexpr (KIND == 2 && LEAN) {
            // a thresholded sink (option "frozen_forced" bit 2): UPR = -d sms / d c of the wave's own column, at the rows where the
            // launch path evaluates the Jacobian anew, from the state at the step start (its own y_new of the row before, or the
            // year's input) and the file source at the row's Jacobian time -- jac_core's expressions, into the plane P.UPR names
            // (the cache's own).  The row's phases read it through line_diag_from: the wave's own stores, read back by itself
            // (every wave of a team forms the column for itself: the same values to the same places)
            if (A.upr_on != 0 && uni_i(R.upr) != 0 && col_wave) {
                const double* sp = PIECES ? T.SRC : A.SRC + (size_t)i * A.C.np;
                forced_upr_col<E, MPX>(P, FZ_Y, sp, const_cast<double*>(P.UPR), wave % P.ny, lane);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        // SciPy's error estimate on this step too (every "frozen_err_check"-th: the host compares it with what the recorded
        // step was accepted with).  Three phases of their own, one wave per column: the tendency at the step start before the
        // Newton iterations, the estimate behind the last of them -- which is then an ordinary iteration --, the end of the step
        const bool with_err = uni_i(R.err) != 0 && !last_row && i > 0;
        if (with_err) {
            if (col_wave && (!TEAM || tw == 0))
                tend_at_body<E, KIND, MPX>(P, FZ_Y, PIECES ? kv_prev : A.C.KV + ((size_t)(i - 1) * 3 + 2) * A.C.kv_len, A.F, wave, lane);
            FZ_SYNC()
        }
        for (int k = 0; k < n_iter; ++k) {
            int src = 0;
            for (int it = 0; it < m; ++it) {
                const bool do_stage = it == 0, first = it == 0, do_update = it == m - 1, delta = m == 2;
                const bool is_final = do_update && k == n_iter - 1 && !last_row && !with_err;
                FusedArgs FA = {};
                FA.st.y = FZ_Y; FA.st.z = FZ_Z; FA.st.w = A.W;
                FA.st.zout = (do_stage && do_update) ? FZ_ZN : FZ_Z;
                FA.st.kv[0] = kvb; FA.st.kv[1] = kvb + A.C.kv_len; FA.st.kv[2] = kvb + 2 * A.C.kv_len;
                FA.st.br = A.BR; FA.st.bcr = A.BCR; FA.st.bci = A.BCI;
                FA.st.nv = nv; FA.st.mreal = R.mreal; FA.st.mcr = R.mcr; FA.st.mci = R.mci;
                FA.sw.JL = J; FA.sw.JU = J + A.C.np; FA.sw.JS = J + 2 * A.C.np; FA.sw.JN = J + 3 * A.C.np; FA.sw.JC = J + 4 * A.C.np;
                // LEAN: this phase factorises (the first of the row); the one row of tables
                const bool fac = LEAN != 0 && k == 0 && it == 0;
                // (The factorising bodies read the grid's parameters where the launch put them, in the kernel-argument segment, whose
                // first argument P is: with them reading the kernel's own copy of P, the compiler -- ROCm 7.2's clang 22, instcombine's
                // rewrite of an argument copy that is only read -- crashes on the forced module at one level per lane.  Same values.)
                const DevP& PK = *(const DevP*)__builtin_amdgcn_kernarg_segment_ptr();
                (void)PK;
                if constexpr (LEAN) {
                    FA.sw.fr_inv = A.C.fr_inv; FA.sw.fc_invr = A.C.fc_invr; FA.sw.fc_invi = A.C.fc_invi;
                    FA.sw.fr_tab = A.C.fr_tab; FA.sw.fc_tabr = A.C.fc_tabr; FA.sw.fc_tabi = A.C.fc_tabi;
                    FA.sw.cre = R.cre; FA.sw.ccr = R.ccr; FA.sw.cci = R.cci;
                } else if constexpr (PIECES) {
                    FA.sw.fr_inv = T.fr_inv; FA.sw.fc_invr = T.fc_invr; FA.sw.fc_invi = T.fc_invi;
                    FA.sw.fr_tab = T.fr_tab; FA.sw.fc_tabr = T.fc_tabr; FA.sw.fc_tabi = T.fc_tabi;
                } else {
                    FA.sw.fr_inv = A.C.fr_inv + (size_t)i * nv; FA.sw.fc_invr = A.C.fc_invr + (size_t)i * nv;
                    FA.sw.fc_invi = A.C.fc_invi + (size_t)i * nv;
                    FA.sw.fr_tab = A.C.fr_tab + (size_t)i * A.C.ntab; FA.sw.fc_tabr = A.C.fc_tabr + (size_t)i * A.C.ntab;
                    FA.sw.fc_tabi = A.C.fc_tabi + (size_t)i * A.C.ntab;
                }
                FA.sw.f32 = 0;
                FA.sw.br = A.BR; FA.sw.bcr = A.BCR; FA.sw.bci = A.BCI;
                FA.sw.xr_old = src ? A.XR[1] : A.XR[0]; FA.sw.xcr_old = src ? A.XCR[1] : A.XCR[0];
                FA.sw.xci_old = src ? A.XCI[1] : A.XCI[0];
                FA.sw.xr_new = src ? A.XR[0] : A.XR[1]; FA.sw.xcr_new = src ? A.XCR[0] : A.XCR[1];
                FA.sw.xci_new = src ? A.XCI[0] : A.XCI[1];
                FA.sw.first = first ? 1 : 0;
                // (the year's check reads the norms of a step's last two iterations; the partials of the others went to a scratch
                // row nobody read: the wave-per-column body no longer forms them.  The team and the one-wave bodies of one and two
                // levels per lane keep the scratch row)
                FA.part = (k == n_iter - 1) ? A.STEP_PART + (size_t)(3 * i) * P.ncol
                                            : ((k == n_iter - 2) ? A.STEP_PART + (size_t)(3 * i + 1) * P.ncol
                                                                 : ((!TEAM && E >= 3) ? nullptr : A.PART));
                FA.do_stage = do_stage ? 1 : 0; FA.do_update = do_update ? 1 : 0; FA.delta = delta ? 1 : 0;
                if constexpr (COEF_LDS) {
                    if (step_in_lds && lds_step != i) {
                        // first phase of a step: what is constant over the step's iterations goes to LDS once -- the three mixing
                        // columns and JL, JU of the ypos column shared out over the workgroup's waves, each wave's own pivots
                        for (int r = tw; r < 5; r += nwv) {
                            double v[E];
                            // (selects, not an index: a struct indexed at run time would live in scratch memory)
                            const double* src = (r == 0) ? FA.st.kv[0] : ((r == 1) ? FA.st.kv[1] : ((r == 2) ? FA.st.kv[2]
                                                : ((r == 3) ? FA.sw.JL : FA.sw.JU)));
                            load_col<E, MPX>(src, wave % P.ny, lane, v);
                            w_lds_put<E>(step_lds, r, lane, v);
                        }
                        if constexpr (!LEAN) {
                        if (piv_in_lds && col_wave) {
                            double v[E];
                            load_col<E>(FA.sw.fr_inv, wave, lane, v);
                            w_lds_put<E>(my_piv, 0, lane, v);
                        }
                        }       // (LEAN: the pivots do not exist yet -- filled behind the factorising phase below)
                        lds_step = i;
                        __syncthreads();
                    }
                }
#ifdef NK2D_FROZEN_CLOCKS
                late.ck_match = nbs.ck_match;
#endif
                if (is_final) {
                    FinalArgs Fin;
                    Fin.ynew = FZ_YOLD;
                    Fin.znext = do_stage ? FZ_ZN : FZ_Z;
                    Fin.x0 = R.x0; Fin.x1 = R.x1; Fin.x2 = R.x2;
                    Fin.nblk_cols = 0;
#if FZ_ONLY
                    (void)fac;
                    if (col_wave) {
                        const StageXchg XC = {FZ_U, do_stage ? FZ_UN : FZ_U, 0};
                        newton_fused_body<E, KIND, 0, 1, MPX, 1, FZ_ONLY>(P, FA, wave, lane, &Fin, &L, &own, &late, &XC);
                    }
#else
                    if constexpr (TEAM) {
                        if constexpr (LEAN) {
                            if (col_wave && fac)
                                newton_team_body<E, KIND, 1, 1, 4, 1, MPX>(PK, FA, *reinterpret_cast<TeamLds<E, 3>*>(team_lds), wave, tw, lane, &Fin);
                        }
                        if (col_wave && !fac)
                            newton_team_body<E, KIND, 0, 1, 4, 1, MPX>(P, FA, *reinterpret_cast<TeamLds<E, 3>*>(team_lds), wave, tw, lane, &Fin);
                    } else if (col_wave && fac) {
                        if constexpr (LEAN && COEF_LDS) frozen_factor_phase<E, KIND, MPX, 1>(PK, FA, wave, lane, &Fin, &L, A.coef_lds, w_in_lds, piv_in_lds ? my_piv : nullptr);
                        else if constexpr (LEAN) newton_fused_body<E, KIND, 1, 1, MPX, 1>(PK, FA, wave, lane, &Fin);
                    } else if (col_wave) {
                        bool taken = false;
                        if constexpr (KIND == 0 && E <= 2) {
                            if (m == 1) { newton_single_body<E, MPX, 1>(P, FA, wave, lane, &Fin); taken = true; }
                        }
                        if constexpr (OWN) {
                            if constexpr (XCHG) {
                            if (own_bits == 48 && xchg) {
                                const StageXchg XC = {FZ_U, do_stage ? FZ_UN : FZ_U, 0};
                                if constexpr (XLANE) {
                                    if (xlane) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 959>(P, FA, wave, lane, &Fin, &L, &own, &late, &XC); taken = true; }
                                }
                                if (!taken) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 447>(P, FA, wave, lane, &Fin, &L, &own, &late, &XC); taken = true; }
                            }
                            }
                            if (taken) {}
                            else if (own_bits == 48) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 191>(P, FA, wave, lane, &Fin, &L, &own, &late); taken = true; }
                            else if (!PIECES && own_bits == 32) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 47>(P, FA, wave, lane, &Fin, &L, &own); taken = true; }
                            else if (own_bits == 16) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 31>(P, FA, wave, lane, &Fin, &L, &own); FZ_OWN_DEAD() taken = true; }
                        }
                        if constexpr (COEF_LDS) {
                            if (taken) {}
                            else if (step_in_lds && piv_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 15>(P, FA, wave, lane, &Fin, &L); FZ_OWN_DEAD() taken = true; }
                            else if (step_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 7>(P, FA, wave, lane, &Fin, &L); FZ_OWN_DEAD() taken = true; }
                            else if (w_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 3>(P, FA, wave, lane, &Fin, &L); FZ_OWN_DEAD() taken = true; }
                            else if (A.coef_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 1, 1>(P, FA, wave, lane, &Fin, &L); FZ_OWN_DEAD() taken = true; }
                        }
                        if (!taken) { newton_fused_body<E, KIND, 0, 1, MPX, 1>(P, FA, wave, lane, &Fin); FZ_OWN_DEAD() }
                    }
#endif
                    swapY ^= 1;
                    if (do_stage) swapZ ^= 1;
                } else {
#if FZ_ONLY
                    (void)fac;
                    if (col_wave) {
                        // (Z to memory where something reads it from there: the estimate and the end of a step that carries one,
                        // the caller's commit of the last row)
                        const StageXchg XC = {FZ_U, (do_stage && do_update) ? FZ_UN : FZ_U, (with_err || last_row) ? 1 : 0};
                        newton_fused_body<E, KIND, 0, 1, MPX, 0, FZ_ONLY>(P, FA, wave, lane, nullptr, &L, &own, &late, &XC);
                    }
#else
                    if constexpr (TEAM) {
                        if constexpr (LEAN) {
                            if (col_wave && fac)
                                newton_team_body<E, KIND, 1, 1, 4, 0, MPX>(PK, FA, *reinterpret_cast<TeamLds<E, 3>*>(team_lds), wave, tw, lane, nullptr);
                        }
                        if (col_wave && !fac)
                            newton_team_body<E, KIND, 0, 1, 4, 0, MPX>(P, FA, *reinterpret_cast<TeamLds<E, 3>*>(team_lds), wave, tw, lane, nullptr);
                    } else if (col_wave && fac) {
                        if constexpr (LEAN && COEF_LDS) frozen_factor_phase<E, KIND, MPX, 0>(PK, FA, wave, lane, nullptr, &L, A.coef_lds, w_in_lds, piv_in_lds ? my_piv : nullptr);
                        else if constexpr (LEAN) newton_fused_body<E, KIND, 1, 1, MPX, 0>(PK, FA, wave, lane);
                    } else if (col_wave) {
                        bool taken = false;
                        if constexpr (KIND == 0 && E <= 2) {
                            if (m == 1) { newton_single_body<E, MPX, 0>(P, FA, wave, lane); taken = true; }
                        }
                        if constexpr (OWN) {
                            if constexpr (XCHG) {
                            if (own_bits == 48 && xchg) {
                                // (Z to memory where something reads it from there: the estimate and the end of a step that carries one,
                                // the caller's commit of the last row)
                                const StageXchg XC = {FZ_U, (do_stage && do_update) ? FZ_UN : FZ_U, (with_err || last_row) ? 1 : 0};
                                if constexpr (XLANE) {
                                    if (xlane) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 959>(P, FA, wave, lane, nullptr, &L, &own, &late, &XC); taken = true; }
                                }
                                if (!taken) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 447>(P, FA, wave, lane, nullptr, &L, &own, &late, &XC); taken = true; }
                            }
                            }
                            if (taken) {}
                            else if (own_bits == 48) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 191>(P, FA, wave, lane, nullptr, &L, &own, &late); taken = true; }
                            else if (!PIECES && own_bits == 32) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 47>(P, FA, wave, lane, nullptr, &L, &own); taken = true; }
                            else if (own_bits == 16) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 31>(P, FA, wave, lane, nullptr, &L, &own); FZ_OWN_DEAD() taken = true; }
                        }
                        if constexpr (COEF_LDS) {
                            if (taken) {}
                            else if (step_in_lds && piv_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 15>(P, FA, wave, lane, nullptr, &L); FZ_OWN_DEAD() taken = true; }
                            else if (step_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 7>(P, FA, wave, lane, nullptr, &L); FZ_OWN_DEAD() taken = true; }
                            else if (w_in_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 3>(P, FA, wave, lane, nullptr, &L); FZ_OWN_DEAD() taken = true; }
                            else if (A.coef_lds) { newton_fused_body<E, KIND, 0, 1, MPX, 0, 1>(P, FA, wave, lane, nullptr, &L); FZ_OWN_DEAD() taken = true; }
                        }
                        if (!taken) { newton_fused_body<E, KIND, 0, 1, MPX, 0>(P, FA, wave, lane); FZ_OWN_DEAD() }
                    }
#endif
                    if (do_stage && do_update) swapZ ^= 1;
                }
                src = 1 - src;
                if constexpr (OWN) {
                    // the hand-over in two halves: the flag first, then the store nobody waits for, then the poll
                    nbs.publish();
                    if (late.pending) {
                        if (lane == 0) st_mp<MPX>(late.part, late.acc);
                        late.pending = 0;
                    }
#if FZ_ONLY
                    if (!(poll_one ? nbs.wait_one_load() : nbs.wait())) { status = 1; goto finish; }
#else
                    if (!nbs.wait()) { status = 1; goto finish; }
#endif
                } else {
                    FZ_SYNC()
                }
            }
        }
        if (with_err) {
            if (col_wave && (!TEAM || tw == 0)) {
                ErrArgs EA = {};
                EA.sw.JL = J; EA.sw.JU = J + A.C.np; EA.sw.JS = J + 2 * A.C.np; EA.sw.JN = J + 3 * A.C.np; EA.sw.JC = J + 4 * A.C.np;
                EA.sw.fr_inv = LEAN ? A.C.fr_inv : (PIECES ? T.fr_inv : A.C.fr_inv + (size_t)i * nv);
                EA.sw.fr_tab = LEAN ? A.C.fr_tab : (PIECES ? T.fr_tab : A.C.fr_tab + (size_t)i * A.C.ntab);
                EA.sw.xr_old = A.XR[0]; EA.sw.xr_new = A.XR[1];
                EA.f = A.F; EA.z = FZ_Z; EA.y = FZ_Y; EA.nv = nv; EA.h = R.h;
                EA.part = A.STEP_PART + (size_t)(3 * i + 2) * P.ncol;
                EA.stage = 0; EA.last = 1;
                err_fused_body<E, KIND, MPX>(P, EA, wave, lane);
            }
            FZ_SYNC()
            if (col_wave && (!TEAM || tw == 0)) {
                FinalArgs Fin;
                Fin.ynew = FZ_YOLD;
                Fin.znext = FZ_ZN;
                Fin.x0 = R.x0; Fin.x1 = R.x1; Fin.x2 = R.x2;
                Fin.nblk_cols = 0;
                bool tail_done = false;
                if constexpr (XCHG) {
                    if (xchg) { step_tail_body<E, MPX, 1>(FZ_Y, FZ_Z, nv, Fin, A.W, wave, lane, FZ_UN); tail_done = true; }
                }
                if (!tail_done) step_tail_body<E, MPX>(FZ_Y, FZ_Z, nv, Fin, A.W, wave, lane);
                own.valid = 0;      // (this rare phase writes Y and Z: the next stage part takes both from memory -- or Y and its own U)
                if constexpr (COEF_LDS) {
                    if (w_in_lds) {     // (this rare phase writes W to memory: into the column's LDS copy from there)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            double wv[E];
                            load_col<E, (TEAM ? MPX : 0)>(A.W + r * nv, wave, lane, wv);
                            w_lds_put<E>(my_w, r, lane, wv);
                        }
                    }
                }
            }
            swapY ^= 1;
            swapZ ^= 1;
            FZ_SYNC()
        }
        done = i + 1;
    }
finish:
    if constexpr (COEF_LDS) {
        if (w_in_lds && col_wave) {      // W of the last phase back where the launch-per-phase path keeps it
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double wv[E];
                w_lds_get<E>(my_w, r, lane, wv);
                store_col<E>(A.W + r * nv, wave, lane, wv);
            }
        }
    }
    // no barrier behind the last phase: every workgroup reports a failure of its own (the host cleared `out`), the first the
    // rest -- a workgroup that gave up raised the abort flag, its neighbours give up on it in turn
    if (status != 0 && threadIdx.x == 0) A.out[0] = (double)status;
#ifdef NK2D_FROZEN_CLOCKS
    // probe build: wave 0 of the middle workgroup reports its spans in spare slots of `out` (ticks of 10 ns: the store
    // drains, flag store to poll match, poll match to the stage part's neighbour columns in registers, the whole kernel -- the
    // rest of the phases is the difference) and its phase count
    if (wg == (int)(gridDim.x / 2) && threadIdx.x == 0) {
        A.out[8] = (double)nbs.ck_drain; A.out[9] = (double)nbs.ck_wait;
        A.out[10] = (double)((long long)__builtin_amdgcn_s_memrealtime() - ck_begin); A.out[11] = (double)nbs.phase;
        A.out[12] = (double)late.ck_fetch;
    }
#endif
    if (wg == 0 && threadIdx.x == 0) {
        A.out[1] = (double)done; A.out[2] = (double)swapY; A.out[3] = (double)swapZ; A.out[4] = (double)nbs.phase;
    }
#undef FZ_SYNC
#undef FZ_OWN_DEAD
#undef FZ_Y
#undef FZ_YOLD
#undef FZ_Z
#undef FZ_ZN
#undef FZ_U
#undef FZ_UN
