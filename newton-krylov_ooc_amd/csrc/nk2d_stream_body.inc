// nk2d_stream_body.inc -- the device side of the command-stream kernel (nk2d_stream.h): the relay, the body of the resident kernel and
// its two entry points.  Included by the translation units that instantiate it: nk2d_stream.hip (today's body, XL = 0, host-fed and tape)
// and nk2d_stream_xl.hip (the flavour of option "stream_xlane"), so that the two sets of instantiations compile side by side.
// ---------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ld_pair_sys(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long ld_pair_dev(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The relay: ONE wave (workgroup 0) polls the host's ring over PCIe -- one reader, whatever the number of workgroups -- and
// forwards every complete command into the ring in HBM, which the workgroups poll.  It leaves behind the EXIT command, or
// when nothing has come for the length of the time limit (the host is gone), raising the abort flag.
__device__ __forceinline__ void stream_relay(const StreamArgs& A, int lane) {
    unsigned seq = A.seq0;
    long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();
    long long spins = 0;
    for (;;) {
        const size_t slot = (size_t)(seq % NK2D_RING_SLOTS) * NK2D_CMD_DWORDS;
        const unsigned long long a = ld_pair_sys(A.h_ring + slot + lane);
        const unsigned long long b = ld_pair_sys(A.h_ring + slot + 64 + lane);
        const unsigned long long d = ld_pair_sys(A.h_ring + slot + 128 + lane);
        // (pair 0 says how many pairs the command has -- once ITS stamp is this command's)
        const unsigned head = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)a, 0);
        const int ndw = ((unsigned)__builtin_amdgcn_readlane((int)(unsigned)(a >> 32), 0) == seq) ? (int)(head >> 16) : NK2D_CMD_DWORDS;
        if (__all((int)(((unsigned)(a >> 32) == seq || lane >= ndw) && ((unsigned)(b >> 32) == seq || 64 + lane >= ndw) &&
                        ((unsigned)(d >> 32) == seq || 128 + lane >= ndw)))) {
            if (lane < ndw) __hip_atomic_store(A.d_ring + slot + lane, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (64 + lane < ndw) __hip_atomic_store(A.d_ring + slot + 64 + lane, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (128 + lane < ndw) __hip_atomic_store(A.d_ring + slot + 128 + lane, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int op = (int)(head & 0xffffu);
            if (op == NK2D_OP_EXIT) return;
            ++seq;
            t_begin = (long long)__builtin_amdgcn_s_memrealtime();
            spins = 0;
            continue;
        }
        const int ab = __builtin_amdgcn_readfirstlane(
            (lane == 0) ? __hip_atomic_load(A.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
        const bool late = ((++spins & 15) == 0 || A.spin_ticks == 0) &&
                          (long long)__builtin_amdgcn_s_memrealtime() - t_begin > A.spin_ticks;
        if (late || ab != 0) {
            if (lane == 0) {
                __hip_atomic_store(A.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(A.h_status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
    }
}

// TAPE (option "frozen_tape"): the commands come from a tape in HBM instead of the ring -- no relay, no stamps, no ring to
// poll, nothing to tell the host.  Wave 0 loads command k+1 into registers when command k starts and puts it into the second
// of two LDS buffers when its part of command k is done; between two commands a workgroup waits for its lateral neighbours
// only.  Everything else -- the device functions, the hand-over, the bounded waits -- is the host-fed kernel's.
// XL (option "stream_xlane"): the helper family of every command's cross-lane moves (nk2d_common.h) -- 0, today's text, or
// NK2D_FROZEN_XLANE_MOVES: distances 1 and 32 and the wave sums in the VALU.  A flavour of its own, chosen by the host when the
// kernel starts; the tape flavour has XL = 0 only.
template <int E, int KIND, bool TAPE, int XL = 0>
__device__ __forceinline__ void stream_body(const DevP& P, const StreamArgs& A) {
    static_assert(XL == 0 || (XL == NK2D_FROZEN_XLANE_MOVES && !TAPE), "the helper families of the command stream");
    constexpr int XC = (XL != 0) ? 512 : 0;      // (CL bit 9 of newton_fused_body)
    __shared__ int lds_ok;
    __shared__ StreamCmd cmdb[TAPE ? 2 : 1];
    int cur = 0;
    const int lane = threadIdx.x & 63;
    const int tw = uni_i((int)(threadIdx.x >> 6));          // the wave's place in its workgroup = its tracer
    if (!TAPE && blockIdx.x == 0) {
        // (no relay where the host writes its commands straight into the ring in HBM)
        if (tw == 0 && A.h_ring != nullptr) stream_relay(A, lane);
        return;
    }
    const int wg = TAPE ? (int)blockIdx.x : (int)blockIdx.x - 1;
    const int nw = (int)(blockDim.x >> 6);
    const int j0 = wg * A.cpw, j1 = min(j0 + A.cpw, P.ny);   // this workgroup's ypos columns, every tracer of them
    const int left = (wg > 0) ? wg - 1 : -1, right = (wg < A.nwg - 1) ? wg + 1 : -1;
    // the static coefficients of this workgroup's ypos columns (the same for every tracer of a column) in LDS for as long as the
    // kernel runs: otherwise fetched from L2 by every Newton command (see load_coef_lds)
    // ... and W of its columns (every tracer): the wave's own, read and rewritten by every Newton command and by nothing else of
    // this kernel but the predictions of SETUP / BOUNDARY -- loaded when the kernel starts, stored back when it ends (what runs
    // between two kernels of a year finds it in memory)
    extern __shared__ double dyn_lds[];
    const bool w_in_lds = (A.coef_lds & 2) != 0;
    double* const w_base = dyn_lds + (size_t)A.cpw * NK2D_COEF_LDS_DOUBLES(E);
    const size_t nvw = (size_t)P.ncol * (E * 64);
#define ST_WLDS(tr, j) (w_base + ((size_t)((j) - j0) * P.tc + (tr)) * (3 * E * 64))
    auto w_from_memory = [&](int tr, int j) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double wv[E];
            load_col<E>(A.W + r * nvw, tr * P.ny + j, lane, wv);
            w_lds_put<E>(ST_WLDS(tr, j), r, lane, wv);
        }
    };
    if (A.coef_lds) {
        for (int j = j0 + tw; j < j1; j += nw) {
            ColCoef<E> cf;
            load_coef<E>(P, j, lane, cf);
            store_coef_lds<E>(dyn_lds + (size_t)(j - j0) * NK2D_COEF_LDS_DOUBLES(E), lane, cf);
        }
        if (w_in_lds)
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) w_from_memory(tr, j);
        __syncthreads();
    }
    unsigned seq = A.seq0;
    int status = 0;
    long long t_cmd = 0, t_exec = 0, t_nb = 0, n_cmd = 0;     // where the time of this workgroup goes (wave 0's clock)
    long long t_op[4] = {0, 0, 0, 0}, n_op[4] = {0, 0, 0, 0};
    // Wave 0 waits for two things between two commands, with ONE polling loop: that both lateral neighbours have completed
    // the command this workgroup has just completed, and that the next command is in the ring (every pair of its slot carries
    // its stamp) -- which it then copies into LDS for the workgroup.  Before the first command there is nobody to wait for.
    // Returns (to wave 0's lanes) 1, or 0 when a wait ran over the time limit or another workgroup has given up.
    auto wait_and_fetch = [&](unsigned done_seq, bool with_neighbours, long long& ticks_nb, long long& ticks_cmd) -> int {
        StreamCmd& cmd = cmdb[0];
        const unsigned next = done_seq + 1u;
        const size_t slot = (size_t)(next % NK2D_RING_SLOTS) * NK2D_CMD_DWORDS;
        const int other = with_neighbours ? ((lane == 0) ? left : ((lane == 1) ? right : -1)) : -1;
        bool nb_ok = !with_neighbours;
        long long spins = 0;
        const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();
        long long t_nb_ok = t_begin;
        for (;;) {
            if (!nb_ok) {
                unsigned v = done_seq;
                if (other >= 0) v = __hip_atomic_load(A.flags + (size_t)other * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((int)((int)(v - done_seq) >= 0))) { nb_ok = true; t_nb_ok = (long long)__builtin_amdgcn_s_memrealtime(); }
            }
            if constexpr (TAPE) {      // (the next command is in LDS already)
                if (nb_ok) { ticks_nb += t_nb_ok - t_begin; return 1; }
            } else {
            const unsigned long long a = ld_pair_dev(A.d_ring + slot + lane);
            const unsigned long long b = ld_pair_dev(A.d_ring + slot + 64 + lane);
            const unsigned long long d = ld_pair_dev(A.d_ring + slot + 128 + lane);
            const unsigned head = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)a, 0);
            const int ndw = ((unsigned)__builtin_amdgcn_readlane((int)(unsigned)(a >> 32), 0) == next) ? (int)(head >> 16) : NK2D_CMD_DWORDS;
            if (nb_ok && __all((int)(((unsigned)(a >> 32) == next || lane >= ndw) && ((unsigned)(b >> 32) == next || 64 + lane >= ndw) &&
                                     ((unsigned)(d >> 32) == next || 128 + lane >= ndw)))) {
                unsigned* dw = reinterpret_cast<unsigned*>(&cmd);
                if (lane < ndw) dw[lane] = (lane == 0) ? (head & 0xffffu) : (unsigned)a;
                if (64 + lane < ndw) dw[64 + lane] = (unsigned)b;
                if (128 + lane < ndw) dw[128 + lane] = (unsigned)d;
                const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
                ticks_nb += t_nb_ok - t_begin;
                ticks_cmd += t_end - t_nb_ok;
                return 1;
            }
            }
            const int ab = __builtin_amdgcn_readfirstlane(
                (lane == 0) ? __hip_atomic_load(A.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
            const bool late = ((++spins & 63) == 0 || A.spin_ticks == 0) &&
                              (long long)__builtin_amdgcn_s_memrealtime() - t_begin > A.spin_ticks;
            if (late || ab != 0) {
                if (lane == 0) __hip_atomic_store(A.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return 0;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    // the tape: wave 0's loads of the command at dword `at` (three dwords a lane), and their way into an LDS buffer
    size_t tape_next = 0;
    auto tape_load = [&](size_t at, unsigned& a, unsigned& b, unsigned& d) {
        a = (at + lane < A.tape_dwords) ? A.tape[at + lane] : 0u;
        b = (at + 64 + lane < A.tape_dwords) ? A.tape[at + 64 + lane] : 0u;
        d = (at + 128 + lane < A.tape_dwords) ? A.tape[at + 128 + lane] : 0u;
    };
    auto tape_put = [&](StreamCmd& dst, unsigned a, unsigned b, unsigned d) {
        const unsigned head = (unsigned)__builtin_amdgcn_readlane((int)a, 0);
        const int ndw = min((int)(head >> 16), NK2D_CMD_DWORDS);
        unsigned* dw = reinterpret_cast<unsigned*>(&dst);
        if (lane < ndw) dw[lane] = (lane == 0) ? (head & 0xffffu) : a;
        if (64 + lane < ndw) dw[64 + lane] = b;
        if (128 + lane < ndw) dw[128 + lane] = d;
        tape_next += (size_t)max(ndw, 1);
    };
    if (TAPE) {
        if (tw == 0) {
            unsigned a, b, d;
            tape_load(0, a, b, d);
            tape_put(cmdb[0], a, b, d);
            if (lane == 0) lds_ok = 1;
        }
    } else if (tw == 0) {
        const int good = wait_and_fetch(seq - 1u, false, t_nb, t_cmd);
        if (lane == 0) lds_ok = good;
    }
    __syncthreads();
    if (lds_ok == 0) status = 1;
    while (status == 0) {
        const long long t1 = (long long)__builtin_amdgcn_s_memrealtime();
        StreamCmd& cmd = cmdb[cur];
        const int op = uni_i(cmd.op), flags = uni_i(cmd.flags);
        if (op == NK2D_OP_EXIT) {
            if (threadIdx.x == 0)
                __hip_atomic_store(A.flags + (size_t)wg * 32, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        unsigned ta = 0, tb = 0, td = 0;     // (the tape: the next command, on its way while this one executes)
        if (TAPE && tw == 0) tape_load(tape_next, ta, tb, td);
        // ---- its work on this workgroup's columns: wave tw takes tracer tw (a one-wave workgroup every tracer in turn)
        if (op == NK2D_OP_NEWTON) {
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    const LdsSrc L = {dyn_lds + (size_t)(j - j0) * NK2D_COEF_LDS_DOUBLES(E), w_in_lds ? ST_WLDS(tr, j) : nullptr, nullptr, nullptr};
                    if (w_in_lds) {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 0, 3 | XC>(P, cmd.u.nf, tr * P.ny + j, lane, nullptr, &L);
                        else newton_fused_body<E, KIND, 0, 1, 1, 0, 3 | XC>(P, cmd.u.nf, tr * P.ny + j, lane, nullptr, &L);
                    } else if (A.coef_lds) {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 0, 1 | XC>(P, cmd.u.nf, tr * P.ny + j, lane, nullptr, &L);
                        else newton_fused_body<E, KIND, 0, 1, 1, 0, 1 | XC>(P, cmd.u.nf, tr * P.ny + j, lane, nullptr, &L);
                    } else {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 0, XC>(P, cmd.u.nf, tr * P.ny + j, lane);
                        else newton_fused_body<E, KIND, 0, 1, 1, 0, XC>(P, cmd.u.nf, tr * P.ny + j, lane);
                    }
                }
        } else if (op == NK2D_OP_NEWTON_FINAL) {
            // the last Newton iteration of a frozen step, which also ends the step (y_new, the next attempt's predicted stage
            // values), and the next attempt's planes -- into the second sets of plane buffers: this command's own stage and sweep
            // parts still read the current ones
            const StreamFinal& S = cmd.u.fn;
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    const LdsSrc L = {dyn_lds + (size_t)(j - j0) * NK2D_COEF_LDS_DOUBLES(E), w_in_lds ? ST_WLDS(tr, j) : nullptr, nullptr, nullptr};
                    if (w_in_lds) {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 1, 3 | XC>(P, S.nf, tr * P.ny + j, lane, &S.fin, &L);
                        else newton_fused_body<E, KIND, 0, 1, 1, 1, 3 | XC>(P, S.nf, tr * P.ny + j, lane, &S.fin, &L);
                    } else if (A.coef_lds) {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 1, 1 | XC>(P, S.nf, tr * P.ny + j, lane, &S.fin, &L);
                        else newton_fused_body<E, KIND, 0, 1, 1, 1, 1 | XC>(P, S.nf, tr * P.ny + j, lane, &S.fin, &L);
                    } else {
                        if (flags & NK2D_CMD_FACTOR) newton_fused_body<E, KIND, 1, 1, 1, 1, XC>(P, S.nf, tr * P.ny + j, lane, &S.fin);
                        else newton_fused_body<E, KIND, 0, 1, 1, 1, XC>(P, S.nf, tr * P.ny + j, lane, &S.fin);
                    }
                }
            for (int ti = tw; ti < 3; ti += nw)
                for (int j = j0; j < j1; ++j) {
                    double kv[E];
                    vmix_body_kv<E, 1>(P, S.V, ti * P.ny + j, lane, kv);
                    if (ti == S.J.stage)
                        jac_core<E, 1, XL>(P, kv, S.V.out[ti], S.J.JL, S.J.JU, S.J.JS, S.J.JN, S.J.JC, nullptr, nullptr, j, lane);
                }
        } else if (op == NK2D_OP_ERR) {
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) err_fused_body<E, KIND, 1, XL>(P, cmd.u.err, tr * P.ny + j, lane);
        } else if (op == NK2D_OP_SETUP) {
            // the mixing planes of the attempt's three stage times for this workgroup's columns (the wave that computes the
            // plane of the Jacobian's stage derives the Jacobian planes of the column from it), then the predicted stage values
            const StreamSetup& S = cmd.u.su;
            for (int ti = tw; ti < 3; ti += nw)
                for (int j = j0; j < j1; ++j) {
                    double kv[E];
                    vmix_body_kv<E, 1>(P, S.V, ti * P.ny + j, lane, kv);
                    if (ti == S.J.stage)
                        jac_core<E, 1, XL>(P, kv, S.V.out[ti], S.J.JL, S.J.JU, S.J.JS, S.J.JN, S.J.JC, nullptr, nullptr, j, lane);
                }
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    predict_body<E, 1>(S.A, tr * P.ny + j, lane);
                    if (w_in_lds) {      // (the prediction wrote W to memory: into the column's LDS copy from there)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        w_from_memory(tr, j);
                    }
                }
        } else if (op == NK2D_OP_BOUNDARY) {
            const StreamBoundary& S = cmd.u.bd;
            for (int ti = tw; ti < 3; ti += nw)
                for (int j = j0; j < j1; ++j) {
                    double kv[E];
                    vmix_body_kv<E, 1>(P, S.V, ti * P.ny + j, lane, kv);
                    if (ti == S.B.jac_stage)
                        jac_core<E, 1, XL>(P, kv, S.V.out[ti], S.B.JL, S.B.JU, S.B.JS, S.B.JN, S.B.JC, nullptr, nullptr, j, lane);
                }
            if (S.B.do_jac && tw == nw - 1)
                for (int j = j0; j < j1; ++j) jac_body<E, 1, XL>(P, S.B.kv_new, S.B.JL, S.B.JU, S.B.JS, S.B.JN, S.B.JC, nullptr, nullptr, j, lane);
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    const int task = tr * P.ny + j;
                    if (S.B.with_tend) {
                        commit_tend_body<E, KIND, 1, XL>(P, S.B.y, S.B.z2, S.B.kv_new, S.B.ynew, S.B.f, task, lane);
                    } else {
                        double c[E], t0[E];
                        load_col<E, 1>(S.B.y, task, lane, c);
                        load_col<E, 1>(S.B.z2, task, lane, t0);
#pragma unroll
                        for (int e = 0; e < E; ++e) c[e] = c[e] + t0[e];
                        store_col<E, 1>(S.B.ynew, task, lane, c);
                    }
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's y_new is in memory before it reads it back
                    predict_body<E, 1>(S.A, task, lane);
                    if (w_in_lds) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        w_from_memory(tr, j);
                    }
                }
        }
        else if (op == NK2D_OP_SWEEP) {
            const SweepArgs& S = cmd.u.sw;
            const int nvar = S.ntasks / P.ny, nre = S.nreal / P.ny;
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    if (nre > 0) sweep_body<E, KIND, 1, XL>(P, S, j * nvar + tr, lane);
                    if (nvar > nre) sweep_body<E, KIND, 1, XL>(P, S, j * nvar + nre + tr, lane);
                }
        } else if (op == NK2D_OP_JAC) {
            const StreamJac& S = cmd.u.jac;
            if (tw == 0)
                for (int j = j0; j < j1; ++j) jac_body<E, 1, XL>(P, S.kvp, S.JL, S.JU, S.JS, S.JN, S.JC, S.ylin, S.UPR, j, lane);
        } else if (op >= NK2D_OP_ERR_RHS && op <= NK2D_OP_COPY) {
            const StreamColumns& S = cmd.u.col;
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) {
                    const int task = tr * P.ny + j;
                    if (op == NK2D_OP_ERR_RHS) err_rhs_body<E, 1>(S.a, S.b, S.nv, S.h, S.out, task, lane);
                    else if (op == NK2D_OP_ERR_RHS2) err_rhs2_body<E, KIND, 1, XL>(P, S.a, S.b, S.c, S.d, S.nv, S.h, S.out, task, lane);
                    else if (op == NK2D_OP_ERR_NORM) err_norm_body<E, 1, XL>(P, S.a, S.b, S.c, S.part, task, lane);
                    else {
                        double v[E];
                        load_col<E, 1>(S.a, task, lane, v);
                        store_col<E, 1>(S.out, task, lane, v);
                    }
                }
        } else if (op == NK2D_OP_DENSE_OUT) {
            const StreamDense& S = cmd.u.dn;
            for (int tr = tw; tr < P.tc; tr += nw)
                for (int j = j0; j < j1; ++j) dense_body<E, 1>(S.yold, S.zp, S.nv, S.x, S.out, tr * P.ny + j, lane);
        }
        // ---- hand-over: every wave has drained its write-through stores, the workgroup publishes the command it has
        // completed (and, where the host waits for it, stamps pinned memory), waits for its two lateral neighbours and
        // for the next command
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (TAPE && tw == 0) tape_put(cmdb[cur ^ 1], ta, tb, td);
        if (A.fences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        const long long t2 = (long long)__builtin_amdgcn_s_memrealtime();
        if (tw == 0) {
            if (lane == 0) {
                __hip_atomic_store(A.flags + (size_t)wg * 32, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!TAPE && (flags & NK2D_CMD_NOTIFY)) __hip_atomic_store(A.h_done + wg, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            const int good = wait_and_fetch(seq, true, t_nb, t_cmd);
            if (lane == 0) lds_ok = good;
        }
        __syncthreads();
        if (A.fences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (lds_ok == 0) { status = 1; break; }
        t_exec += t2 - t1; ++n_cmd;
        {
            const int bucket = (op == NK2D_OP_NEWTON_FINAL) ? 1 : ((op >= 2 && op <= 5) ? op - 2 : -1);
            if (bucket >= 0) { t_op[bucket] += t2 - t1; ++n_op[bucket]; }
        }
        ++seq;
        if (TAPE) cur ^= 1;
    }
    if (w_in_lds) {      // W back to memory: whatever runs behind this kernel (launches, the next kernel of the year) finds it there
        for (int tr = tw; tr < P.tc; tr += nw)
            for (int j = j0; j < j1; ++j) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    double wv[E];
                    w_lds_get<E>(ST_WLDS(tr, j), r, lane, wv);
                    store_col<E>(A.W + r * nvw, tr * P.ny + j, lane, wv);
                }
            }
    }
#undef ST_WLDS
    if (A.prof && threadIdx.x == 0) {
        unsigned long long* pr = A.prof + (size_t)wg * 12;
        pr[0] += (unsigned long long)t_cmd; pr[1] += (unsigned long long)t_exec; pr[2] += (unsigned long long)t_nb;
        pr[3] += (unsigned long long)n_cmd;
        for (int i = 0; i < 4; ++i) { pr[4 + i] += (unsigned long long)t_op[i]; pr[8 + i] += (unsigned long long)n_op[i]; }
    }
    if (status != 0 && threadIdx.x == 0) {
        A.out[0] = (double)status;
        __hip_atomic_store(A.h_status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (wg == 0 && threadIdx.x == 0) A.out[1] = (double)seq;
}

template <int E, int KIND, bool TAPE, int XL = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) k_stream(DevP P, StreamArgs A) {
    stream_body<E, KIND, TAPE, XL>(P, A);
}
// The same within 256 registers, so that a SIMD holds TWO waves (option "stream_two_waves"; phosphorus from five levels per
// lane, where a wave of k_stream holds 280 - 390 registers and the chip therefore 1 024 waves: the 1 248 (tracer, ypos)
// columns of phosphorus at 416 x 416 are then two rounds per command on half as many workgroups).  What does not fit the
// registers lives in scratch memory.
template <int E, int KIND, bool TAPE, int XL = 0>
__global__ void __launch_bounds__(NK2D_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) k_stream_w2(DevP P, StreamArgs A) {
    stream_body<E, KIND, TAPE, XL>(P, A);
}

