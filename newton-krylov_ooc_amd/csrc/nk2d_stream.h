// nk2d_stream.h -- the forward year as a COMMAND STREAM (nk2d_stream.hip).
//
// The host-controlled year (nk2d_radau.hip) is a sequence of launches: attempt set-up, fused Newton iterations, error
// estimate, step boundary -- 24 000 of them per free-running 416 x 416 year, each a launch boundary at which 832 waves wait
// for the slowest of them, and a host round trip per Newton iteration.  Here the same sequence is a stream of COMMANDS -- a
// command is the argument block of the launch it replaces -- executed by ONE resident kernel: a workgroup owns a block of
// ypos columns with all their tracers for as long as the kernel runs, executes command after command with the device
// functions of the per-phase kernels (nk2d_bodies.h: the same bits), and between two commands waits for its two lateral
// neighbours only (a column reads what the columns to its left and right wrote in the command before, and nothing else of
// another workgroup).  The controller stays where it is, on the host, with its decisions, its speculation (the next Newton
// iteration or the error estimate queued before the verdict on this one) and its roll-back by pointer swap: it pushes
// commands into a ring in pinned host memory, a relay wave of the kernel copies them into HBM, and the per-column norm
// partials come back through pinned host memory with a completion stamp per workgroup -- no launch, no event, no
// stream synchronisation inside a year.  Whatever has no command ends the kernel, runs as ordinary launches and the next
// command starts the kernel again.  History samples have one with option "stream_hist" (NK2D_OP_DENSE_OUT: the dense output
// of the step just taken, packed, into a slot of a sample buffer in HBM that the host unpacks and copies out once the
// kernel has ended); without the option a sampled step is such a piece of launches, as the year's last step always is.
#pragma once

#include "nk2d_bodies.h"

#include <vector>

enum { NK2D_OP_EXIT = 1, NK2D_OP_SETUP = 2, NK2D_OP_NEWTON = 3, NK2D_OP_ERR = 4, NK2D_OP_BOUNDARY = 5,
       // the several-sweep error estimate and the second estimate of a rejected step, launch for launch
       NK2D_OP_SWEEP = 6, NK2D_OP_ERR_RHS = 7, NK2D_OP_ERR_RHS2 = 8, NK2D_OP_ERR_NORM = 9, NK2D_OP_COPY = 10,
       // the launch that ends the last Newton iteration of a frozen step and the step (nk2d_r_newton_final)
       NK2D_OP_NEWTON_FINAL = 11,
       // Jacobian planes from a mixing plane in memory (nk2d_k_jac: modules whose Jacobian reads the state)
       NK2D_OP_JAC = 12,
       // a history sample: the dense output of the step just taken (nk2d_r_dense), packed, column by column
       NK2D_OP_DENSE_OUT = 13 };
#define NK2D_CMD_NOTIFY 1   /* the host waits for this command: completion stamp of every workgroup to pinned memory */
#define NK2D_CMD_FACTOR 2   /* OP_NEWTON: the launch that computes the line factorisation of its column (first after an "LU" event) */

struct StreamSetup {        // nk2d_r_attempt_setup
    VmixArgs V;
    PredictArgs A;
    JacOut J;
};
struct StreamBoundary {     // nk2d_r_step_boundary
    VmixArgs V;
    BoundaryArgs B;
    PredictArgs A;
};
struct StreamColumns {      // nk2d_r_err_rhs / _err_rhs2 / _err_norm, a column-wise copy: operands by position
    const double *a, *b, *c, *d;
    double *out, *part;
    size_t nv;
    double h;
};
struct StreamJac {          // nk2d_k_jac
    const double* kvp;
    double *JL, *JU, *JS, *JN, *JC;
    const double* ylin;
    double* UPR;
};
struct StreamDense {        // nk2d_r_dense
    const double *yold, *zp;
    size_t nv;
    double x;
    double* out;
};
struct StreamFinal {        // nk2d_r_newton_final
    FusedArgs nf;
    FinalArgs fin;
    VmixArgs V;
    JacOut J;
};
struct StreamCmd {
    int op, flags;
    union {
        StreamFinal fn;
        StreamJac jac;
        SweepArgs sw;       // nk2d_k_sweep
        StreamColumns col;
        StreamDense dn;
        FusedArgs nf;       // nk2d_r_newton_fused
        ErrArgs err;        // one launch of nk2d_r_err_fused
        StreamSetup su;
        StreamBoundary bd;
    } u;
};

// A ring slot is NK2D_CMD_DWORDS pairs (stamp << 32 | payload dword), each written and read with ONE 8-byte access: a
// reader that finds the expected stamp in every pair has the whole command, whatever order the pairs arrived in -- no fence,
// no flag to order against, on the PCIe hop (host -> relay wave) as on the device (relay wave -> workgroups).
#define NK2D_CMD_DWORDS 192
#define NK2D_RING_SLOTS 256
static_assert(sizeof(StreamCmd) <= 4 * NK2D_CMD_DWORDS, "a command must fit a ring slot");

// Option "stream_xlane": the classes (levels per lane E, module kind, W2 = the two-waves flavour k_stream_w2) whose resident kernel
// exists in the flavour whose cross-lane moves at distances 1 and 32, and wave sums, go through the VALU (template parameter XL of
// stream_body; the tape flavour never).  A class left out here runs today's kernel and reports counter "stream_xlane_bits" 0:
// the ones whose XL flavour needs more scratch memory than their XL = 0 sibling.
// Left out: linear sources at one level per lane, one wave to a SIMD -- 20 bytes of scratch per lane against none
// (profiles/r19_stream_xlane_resources.log).
#define NK2D_STREAM_XLANE(E, KIND, W2) (!((E) == 1 && (KIND) == 0 && !(W2)))

// (the two-waves flavour is instantiated where it can matter: state-dependent sources from five levels per lane)
template <int E, int KIND>
constexpr bool kStreamHasTwoWaves = KIND == 1 && E >= 5;

struct StreamArgs {
    const unsigned long long* h_ring;   // pinned host memory: what the host pushes
    unsigned long long* d_ring;         // HBM: what the relay wave has forwarded
    unsigned* flags;                    // [nwg][32]: commands completed, one 128-byte line per workgroup
    int* abort_flag;
    unsigned* h_done;                   // pinned: [nwg] completion stamps of the commands flagged NOTIFY
    unsigned* h_status;                 // pinned: [0] != 0 once a workgroup or the relay has given up
    double* out;                        // [8]: status, commands completed by workgroup 0
    unsigned seq0;                      // stamp of the first command of this launch
    int nwg, cpw;                       // workgroups, ypos columns per workgroup
    long long spin_ticks;               // longest wait (ticks of s_memrealtime, 100 MHz)
    int fences;
    int coef_lds;                       // bit 0: the static coefficients of the workgroup's ypos columns live in LDS (dynamic shared
                                        // memory), bit 1: so does W of its columns
    double* W;                          // the context's W (3 nv): loaded into LDS when the kernel starts, stored back when it ends
    unsigned long long* prof;           // [nwg][12]: ticks waiting for a command, executing, waiting for neighbours; commands; per op
    const unsigned* tape;               // the tape flavour (k_stream<..., true>): the year's commands in HBM, packed, EXIT last
    size_t tape_dwords;
};

// A frozen year recorded as commands (option "frozen_tape"): what nk2d_stream_push would have written to the ring, packed by
// cmd_dwords (dword 0: op | dwords << 16), in HBM, read by the resident kernel itself -- no host in the loop.  Besides the
// commands it keeps what the controller left behind on the host, so that a year run from the tape ends where the recorded
// controller ended: the roles of the context's buffers before and after, the step's last commit (a launch behind the tape),
// the counters the year books, the rows whose error estimate was evaluated.
struct nk2d_tape_ptrs {
    double *Y, *YOLD, *Z, *ZP, *ZN, *ZS, *KV[5], *KVN[3], *J[5], *JB[5];
};
struct nk2d_tape {
    uint64_t key = 0;                   // schedule key ^ nk2d_fingerprint ^ frozen_err_check (nk2d_frozen_key); 0: none
    uint64_t refused = 0;               // a schedule whose year cannot be taped (a launch with no command inside it)
    int64_t rows = 0;
    std::vector<unsigned> cmds;         // host copy, packed
    int64_t ncmd = 0;                   // commands, EXIT included
    unsigned* dev = nullptr;
    size_t dev_dwords = 0;              // allocated
    nk2d_tape_ptrs p0 = {}, p1 = {};    // buffer roles when the tape starts / after the year
    std::vector<const void*> fixed;     // every other buffer of the context a command may point at, when it was recorded
    double* zero_z = nullptr;           // Z and W zeroed before the first step (the first step has no dense output)
    double* zero_w = nullptr;
    double first_times[3] = {0, 0, 0};  // ... and the mixing planes of its stage times, a launch before the tape (no command)
    double* first_out[3] = {nullptr, nullptr, nullptr};
    const double *fin_y = nullptr, *fin_z2 = nullptr;   // the last step's commit: fin_out <- fin_y + fin_z2, a launch
    double* fin_out = nullptr;
    nk2d_stats st = {};                 // what the recorded year booked
    int64_t sweep_launches = 0, shape_cnt[4] = {0, 0, 0, 0};
    double fused_bytes = 0.0, shape_bytes[4] = {0, 0, 0, 0};
    double lu[3] = {0, 0, 0};
    int factor_pending = 0;
    std::vector<char> err_done;
    double ctl[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the controller's state after the year (nk2d_radau.hip)
    int ctl_i[6] = {0, 0, 0, 0, 0, 0};
};

// host side (nk2d_stream.hip; what the integrator itself calls is declared in nk2d_common.h)
int nk2d_stream_push(nk2d_ctx* c, StreamCmd& cmd, bool notify, unsigned* seq_out = nullptr);
int nk2d_stream_wait(nk2d_ctx* c, unsigned seq);
unsigned nk2d_stream_last_seq(const nk2d_ctx* c);
// the tape: upload after recording, run (0; NK2D_RC_STREAM_LOST when the kernel gave up, 1 when it cannot be resident)
int nk2d_tape_upload(nk2d_ctx* c, nk2d_tape* T);
int nk2d_tape_run(nk2d_ctx* c, nk2d_tape* T);
#ifdef __HIPCC__
// nk2d_stream_xl.hip: the host-fed resident kernel in the flavour of option "stream_xlane", launched on the context's stream -- or,
// with max_blocks, the occupancy query for it; hipErrorInvalidValue for a class NK2D_STREAM_XLANE leaves out
hipError_t nk2d_stream_launch_xl(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, StreamArgs& A, int* max_blocks, size_t lds_bytes, bool two_waves);
#endif
