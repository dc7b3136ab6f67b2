// nk2d_stream.hip -- the forward year as a command stream: one resident kernel executes the launches of the host-controlled
// Radau year (nk2d_radau.hip) as commands; see nk2d_stream.h.  Replaces, for the year that produces F(x)
// (/root/reference/nk_ooc/py_driver_2d/model_state.py:102-114, scipy/integrate/_ivp/radau.py:399-539), the launch per phase
// and the stream synchronisation per Newton iteration -- not the controller, which is the host's, decision for decision.
#include "nk2d_stream.h"

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <vector>

#define NK2D_PART_RING 16

#include "nk2d_stream_body.inc"

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
struct nk2d_stream_state {
    unsigned long long* h_ring = nullptr;   // pinned
    unsigned* h_done = nullptr;             // pinned [nwg]
    unsigned* h_status = nullptr;           // pinned [16]
    unsigned long long* d_ring = nullptr;
    char* d_sync = nullptr;                 // abort flag at 0, workgroup flags from 4096 (one 128-byte line each)
    double* d_out = nullptr;
    unsigned long long* d_prof = nullptr;   // [nwg][4], see StreamArgs
    double* h_out = nullptr;                // pinned [8]
    unsigned seq = 0;                       // stamp of the last command pushed
    unsigned done_upto = 0;                 // every workgroup is known to have completed this command
    std::deque<unsigned> notifies;          // commands flagged NOTIFY that have not been waited for yet
    bool running = false, lost = false;
    bool coef_lds = true;                   // the static coefficients of a workgroup's columns in LDS (NK2D_STREAM_COEF_LDS=0: not)
    bool direct = false;                    // the host writes its commands straight into d_ring (large BAR): no relay hop
    int nwg = 0, cpw = 1, nw = 1;
    bool two_waves = false;                 // k_stream_w2 (two waves to a SIMD) instead of k_stream
    int ncu = 0;                            // compute units of the device
    int xl_fits = -1;                       // option "stream_xlane": the XL flavour keeps the whole grid resident at this shape (-1: not asked yet)
    int turn_waves = 0;                     // what the running kernel holds of the process-wide turn
    int64_t launches = 0;
    // pinned buffers for the norm partials, handed out in turn: the controller names its buffers (hPART, hPARTB, ...) and
    // reuses a name as soon as IT is done with it -- also when a command writing there was dropped unread (an iteration
    // queued ahead of a verdict) and may not have run yet.  A launch boundary used to order that; here every command with
    // partials gets the next buffer of a ring, its name resolves to that buffer until the name is used again, and a buffer
    // comes round again only NK2D_PART_RING commands with partials later.
    double* pbuf[NK2D_PART_RING] = {nullptr};
    int pnext = 0;
    struct { const double* name; double* buf; } pmap[NK2D_PART_RING] = {};
};

// ONE command-stream kernel at a time in a process: two of them do not fit the chip together (a kernel holds a SIMD per
// wave), and a kernel that is only partly resident waits for workgroups that cannot start.  Held from the launch to the
// EXIT command; contexts driven by other host threads wait their turn (their years then run back to back).
namespace {
std::mutex g_turn_mutex;
std::condition_variable g_turn_cv;
int g_turn_waves = 0;          // waves of the resident kernels running now
int g_turn_kernels = 0;
const int kTurnCapacity = 640; // waves that may be resident together (of 1 024 SIMDs, a wave each at the registers these kernels hold)
}  // namespace
// Resident kernels (a one-launch year, a command-stream kernel) wait inside for workgroups that must all be on the chip: a
// process runs them one at a time -- or side by side where their waves together leave the chip room (small grids: a few dozen
// waves each; the years of several tracer modules then overlap as their launches used to).  `waves`: what the kernel holds;
// given back with the same number.  Contexts driven by other host threads wait their turn.
void nk2d_turn_take(int waves) {
    std::unique_lock<std::mutex> lk(g_turn_mutex);
    g_turn_cv.wait(lk, [waves] { return g_turn_kernels == 0 || g_turn_waves + waves <= kTurnCapacity; });
    g_turn_waves += waves;
    g_turn_kernels += 1;
}
void nk2d_turn_give(int waves) {
    {
        std::lock_guard<std::mutex> lk(g_turn_mutex);
        g_turn_waves -= waves;
        g_turn_kernels -= 1;
    }
    g_turn_cv.notify_all();
}

bool nk2d_stream_running(const nk2d_ctx* c) { return c->strm && c->strm->running; }
// the shape of the context's resident kernel (0 before its first year as a command stream): ypos columns per workgroup, and
// whether it is the flavour with two waves to a SIMD
int nk2d_stream_columns_per_workgroup(const nk2d_ctx* c) { return c->strm ? c->strm->cpw : 0; }
int nk2d_stream_two_waves(const nk2d_ctx* c) { return (c->strm && c->strm->two_waves) ? 1 : 0; }
unsigned nk2d_stream_last_seq(const nk2d_ctx* c) { return c->strm ? c->strm->seq : 0u; }

// which contexts run their years as command streams: every module kind, host-side decisions (no norm hook: a sharded module's
// controller waits for all-reduces), double precision factor tables
int nk2d_stream_eligible(const nk2d_ctx* c) {
    if (!c->stream_years || c->stream_lost >= 2 || c->norm_hook || c->factor_fp32) return 0;
    return 1;
}

template <int E, int KIND, bool TAPE>
static hipError_t stream_launch_one(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, StreamArgs& A, int* max_blocks, size_t lds_bytes,
                                    bool two_waves) {
    if constexpr (kStreamHasTwoWaves<E, KIND>) {
        if (two_waves) {
            if (max_blocks) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, k_stream_w2<E, KIND, TAPE>, (int)block.x, lds_bytes);
            hipLaunchKernelGGL((k_stream_w2<E, KIND, TAPE>), grid, block, lds_bytes, c->stream_, P, A);
            return hipGetLastError();
        }
    } else if (two_waves) {
        return hipErrorInvalidValue;
    }
    if (max_blocks) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, k_stream<E, KIND, TAPE>, (int)block.x, lds_bytes);
    hipLaunchKernelGGL((k_stream<E, KIND, TAPE>), grid, block, lds_bytes, c->stream_, P, A);
    return hipGetLastError();
}
// (xlane: the flavour of option "stream_xlane", instantiated in nk2d_stream_xl.hip; the tape flavour has today's body only)
static hipError_t stream_launch(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, StreamArgs& A, int* max_blocks, size_t lds_bytes,
                                bool two_waves, bool tape = false, bool xlane = false) {
    hipError_t rc = hipErrorInvalidValue;
    if (xlane) return tape ? rc : nk2d_stream_launch_xl(c, grid, block, P, A, max_blocks, lds_bytes, two_waves);
    if (tape) {
        NK2D_DISPATCH_EK(c->E, c->kind, rc = (stream_launch_one<EE, KK, true>(c, grid, block, P, A, max_blocks, lds_bytes, two_waves)));
    } else {
        NK2D_DISPATCH_EK(c->E, c->kind, rc = (stream_launch_one<EE, KK, false>(c, grid, block, P, A, max_blocks, lds_bytes, two_waves)));
    }
    return rc;
}
// dynamic shared memory of a launch whose workgroups own cpw ypos columns each
static size_t stream_lds_bytes(const nk2d_ctx* c, int cpw, bool coef_lds) {
    return coef_lds ? sizeof(double) * (size_t)cpw * (NK2D_COEF_LDS_DOUBLES(c->E) + (size_t)c->tc * 3 * c->E * 64) : 0;
}

static int stream_alloc(nk2d_ctx* c) {
    if (c->strm) return 0;
    nk2d_stream_state* S = new nk2d_stream_state();
    c->strm = S;
    S->nw = std::min(c->tc, NK2D_WAVES_PER_BLOCK);
    // ypos columns per workgroup: one where the chip holds a workgroup per column, more where it does not
    DevP P = make_devp(c);
    StreamArgs A = {};
    hipDeviceProp_t prop;
    NK2D_CHECK(c, hipGetDeviceProperties(&prop, c->dev));
    S->ncu = prop.multiProcessorCount;
    S->coef_lds = std::getenv("NK2D_STREAM_COEF_LDS") == nullptr || std::atoi(std::getenv("NK2D_STREAM_COEF_LDS")) != 0;
    // (the columns per workgroup and the LDS they need depend on each other: one column first, more until the grid fits)
    auto columns_per_workgroup = [&](bool two_waves, bool& coef_lds, int& cpw, int& nwg) -> int {
        for (cpw = 1;; ++cpw) {
            int per_cu = 0;
            NK2D_CHECK(c, stream_launch(c, dim3(1), dim3(64 * S->nw), P, A, &per_cu, stream_lds_bytes(c, cpw, coef_lds), two_waves));
            const int capacity = per_cu * prop.multiProcessorCount - 1;     // (one workgroup is the relay's)
            nwg = (c->ny + cpw - 1) / cpw;
            if (capacity >= nwg) return 0;
            if (cpw >= c->ny) {
                if (coef_lds) { coef_lds = false; cpw = 0; continue; }     // (without the LDS copy, then)
                return nk2d_fail(c, "command stream: the kernel does not fit a compute unit");
            }
        }
    };
    NK2D_TRY(columns_per_workgroup(false, S->coef_lds, S->cpw, S->nwg));
    // option "stream_two_waves": where the one-wave-per-SIMD kernel needs several rounds of columns per command and the flavour
    // that fits two waves to a SIMD needs fewer, that one
    // (measured, phosphorus 416 x 416: free-running year 0.728 -> 0.678 s, frozen year 0.374 -> 0.357 s, a Newton command 27.1 ->
    // 19.8 us per workgroup -- profiles/r04_stream_two_waves_phosphorus.log; value 2 takes the flavour wherever it exists: tests)
    if (c->stream_two_waves && c->kind == 1 && c->E >= 5 && (S->cpw > 1 || c->stream_two_waves >= 2)) {
        bool coef2 = S->coef_lds;
        int cpw2 = 0, nwg2 = 0;
        NK2D_TRY(columns_per_workgroup(true, coef2, cpw2, nwg2));
        if ((cpw2 < S->cpw || c->stream_two_waves >= 2) && cpw2 <= S->cpw && coef2 == S->coef_lds) {
            S->two_waves = true; S->cpw = cpw2; S->nwg = nwg2;
        }
    }
    NK2D_CHECK(c, hipHostMalloc((void**)&S->h_ring, sizeof(unsigned long long) * NK2D_RING_SLOTS * NK2D_CMD_DWORDS));
    NK2D_CHECK(c, hipHostMalloc((void**)&S->h_done, sizeof(unsigned) * S->nwg));
    NK2D_CHECK(c, hipHostMalloc((void**)&S->h_status, sizeof(unsigned) * 16));
    NK2D_CHECK(c, hipHostMalloc((void**)&S->h_out, sizeof(double) * 8));
    for (int i = 0; i < NK2D_PART_RING; ++i) NK2D_CHECK(c, hipHostMalloc((void**)&S->pbuf[i], sizeof(double) * c->ncol));
    // Where the device's memory is visible to the host (large BAR), the ring in HBM is a fine-grained allocation the host
    // writes its commands into directly: the pairs cross PCIe once, as posted writes, instead of being fetched by the relay
    // wave's reads.  Otherwise (or with NK2D_STREAM_RELAY=1) the relay.
    S->direct = prop.isLargeBar != 0 && std::getenv("NK2D_STREAM_RELAY") == nullptr;
    if (S->direct) {
        const hipError_t rc = hipExtMallocWithFlags((void**)&S->d_ring, sizeof(unsigned long long) * NK2D_RING_SLOTS * NK2D_CMD_DWORDS,
                                                    hipDeviceMallocFinegrained);
        if (rc != hipSuccess) { (void)hipGetLastError(); S->direct = false; S->d_ring = nullptr; }
    }
    if (!S->direct) NK2D_CHECK(c, hipMalloc((void**)&S->d_ring, sizeof(unsigned long long) * NK2D_RING_SLOTS * NK2D_CMD_DWORDS));
    NK2D_CHECK(c, hipMalloc((void**)&S->d_sync, 4096 + (size_t)S->nwg * 128));
    NK2D_CHECK(c, hipMalloc((void**)&S->d_out, sizeof(double) * 8));
    NK2D_CHECK(c, hipMalloc((void**)&S->d_prof, sizeof(unsigned long long) * 12 * S->nwg));
    NK2D_CHECK(c, hipMemset(S->d_prof, 0, sizeof(unsigned long long) * 12 * S->nwg));
    std::memset(S->h_ring, 0, sizeof(unsigned long long) * NK2D_RING_SLOTS * NK2D_CMD_DWORDS);
    std::memset(S->h_done, 0, sizeof(unsigned) * S->nwg);
    std::memset(S->h_status, 0, sizeof(unsigned) * 16);
    NK2D_CHECK(c, hipMemset(S->d_ring, 0, sizeof(unsigned long long) * NK2D_RING_SLOTS * NK2D_CMD_DWORDS));
    NK2D_CHECK(c, hipMemset(S->d_sync, 0, 4096 + (size_t)S->nwg * 128));
    NK2D_CHECK(c, hipMemset(S->d_out, 0, sizeof(double) * 8));
    return 0;
}

int nk2d_stream_ready(nk2d_ctx* c) { return stream_alloc(c); }

void nk2d_stream_free(nk2d_ctx* c) {
    if (c->tape) {
        (void)hipStreamSynchronize(c->stream_);
        if (c->tape->dev) (void)hipFree(c->tape->dev);
        delete c->tape;
        c->tape = nullptr;
    }
    nk2d_stream_state* S = c->strm;
    if (!S) return;
    if (S->running) (void)nk2d_stream_pause(c);
    (void)hipStreamSynchronize(c->stream_);
    if (S->h_ring) (void)hipHostFree(S->h_ring);
    if (S->h_done) (void)hipHostFree(S->h_done);
    if (S->h_status) (void)hipHostFree(S->h_status);
    if (S->h_out) (void)hipHostFree(S->h_out);
    for (int i = 0; i < NK2D_PART_RING; ++i)
        if (S->pbuf[i]) (void)hipHostFree(S->pbuf[i]);
    if (S->d_ring) (void)hipFree(S->d_ring);
    if (S->d_sync) (void)hipFree(S->d_sync);
    if (S->d_out) (void)hipFree(S->d_out);
    if (S->d_prof) (void)hipFree(S->d_prof);
    delete S;
    c->strm = nullptr;
}

// dwords of a command with this op (the header and the member of the union it uses)
static int cmd_dwords(int op) {
    size_t body = 0;
    switch (op) {
        case NK2D_OP_SETUP: body = sizeof(StreamSetup); break;
        case NK2D_OP_NEWTON: body = sizeof(FusedArgs); break;
        case NK2D_OP_ERR: body = sizeof(ErrArgs); break;
        case NK2D_OP_BOUNDARY: body = sizeof(StreamBoundary); break;
        case NK2D_OP_SWEEP: body = sizeof(SweepArgs); break;
        case NK2D_OP_NEWTON_FINAL: body = sizeof(StreamFinal); break;
        case NK2D_OP_JAC: body = sizeof(StreamJac); break;
        case NK2D_OP_DENSE_OUT: body = sizeof(StreamDense); break;
        case NK2D_OP_EXIT: body = 0; break;
        default: body = sizeof(StreamColumns); break;
    }
    return (int)((offsetof(StreamCmd, u) + body + 3) / 4);
}

// (dword 0 carries the op in its low and the number of dwords in its high half: a reader checks the stamps of that many pairs)
static void ring_write(nk2d_stream_state* S, unsigned seq, const StreamCmd& cmd) {
    unsigned dw[NK2D_CMD_DWORDS] = {0};
    std::memcpy(dw, &cmd, sizeof(StreamCmd));
    const int ndw = cmd_dwords(cmd.op);
    dw[0] = (unsigned)cmd.op | ((unsigned)ndw << 16);
    unsigned long long* slot = (S->direct ? S->d_ring : S->h_ring) + (size_t)(seq % NK2D_RING_SLOTS) * NK2D_CMD_DWORDS;
    for (int k = 0; k < ndw; ++k)
        __atomic_store_n(slot + k, ((unsigned long long)seq << 32) | dw[k], __ATOMIC_RELAXED);
    if (S->direct) __builtin_ia32_sfence();      // (write-combined stores over the BAR: out of the CPU's buffers now)
}

// start the kernel (it will find the commands pushed from now on)
static int stream_start(nk2d_ctx* c) {
    nk2d_stream_state* S = c->strm;
    // option "stream_xlane", read at every start: the flavour whose cross-lane moves go through the VALU, at the shape the context
    // has (its columns per workgroup, its LDS, one or two waves to a SIMD) -- where the class has that flavour and the flavour keeps
    // the whole grid resident at that shape (asked once: the shape does not change); otherwise today's kernel
    bool xlane = false;
    if (c->stream_xlane && NK2D_STREAM_XLANE(c->E, c->kind, S->two_waves ? 1 : 0)) {
        if (S->xl_fits < 0) {
            DevP P0 = make_devp(c);
            StreamArgs A0 = {};
            int per_cu = 0;
            NK2D_CHECK(c, stream_launch(c, dim3(1), dim3(64 * S->nw), P0, A0, &per_cu, stream_lds_bytes(c, S->cpw, S->coef_lds), S->two_waves,
                                        false, true));
            S->xl_fits = (per_cu * S->ncu - 1 >= S->nwg) ? 1 : 0;     // (one workgroup is the relay's)
        }
        xlane = S->xl_fits == 1;
    }
    S->turn_waves = (S->nwg + 1) * S->nw;
    nk2d_turn_take(S->turn_waves);
    StreamArgs A = {};
    A.h_ring = S->direct ? nullptr : S->h_ring; A.d_ring = S->d_ring;
    A.abort_flag = (int*)S->d_sync;
    A.flags = (unsigned*)(S->d_sync + 4096);
    A.h_done = S->h_done; A.h_status = S->h_status; A.out = S->d_out;
    A.seq0 = S->seq + 1;
    A.nwg = S->nwg; A.cpw = S->cpw;
    A.spin_ticks = (long long)(c->barrier_timeout_ms * 1.0e5);
    A.fences = c->year_fences;
    A.prof = S->d_prof;
    A.coef_lds = S->coef_lds ? 3 : 0;
    A.W = c->W;
    DevP P = make_devp(c);
    const hipError_t rc = stream_launch(c, dim3(S->nwg + 1), dim3(64 * S->nw), P, A, nullptr, stream_lds_bytes(c, S->cpw, S->coef_lds),
                                        S->two_waves, false, xlane);
    if (rc != hipSuccess) {
        nk2d_turn_give(S->turn_waves);
        NK2D_CHECK(c, rc);
    }
    c->stream_xlane_bits = xlane ? 1 : 0;
    S->running = true;
    S->launches++;
    c->stream_launches++;
    c->st.nlaunch++;
    return 0;
}

// wait until every workgroup has completed command `seq` (one flagged NOTIFY), bounded by the time limit of the kernel's
// own waits plus a second
int nk2d_stream_wait(nk2d_ctx* c, unsigned seq) {
    nk2d_stream_state* S = c->strm;
    if (!S || S->lost) return NK2D_RC_STREAM_LOST;
    if ((int)(S->done_upto - seq) >= 0) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const double limit_s = 1.0e-3 * c->barrier_timeout_ms + 1.0;
    long long spins = 0;
    for (int wg = 0; wg < S->nwg; ++wg) {
        for (;;) {
            const unsigned v = __atomic_load_n(S->h_done + wg, __ATOMIC_ACQUIRE);
            if ((int)(v - seq) >= 0) break;
            if ((++spins & 255) == 0) {
                const bool gave_up = __atomic_load_n(S->h_status, __ATOMIC_RELAXED) != 0;
                const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (gave_up || waited > limit_s) {
                    // tell the kernel to leave (the relay sees the EXIT, a workgroup stuck in a wait its own time limit),
                    // wait for it, and hand the year back
                    S->lost = true;
                    c->stream_timeouts++;
                    (void)nk2d_stream_pause(c);
                    (void)hipStreamSynchronize(c->stream_);
                    return NK2D_RC_STREAM_LOST;
                }
            }
        }
    }
    S->done_upto = seq;
    while (!S->notifies.empty() && (int)(seq - S->notifies.front()) >= 0) S->notifies.pop_front();
    return 0;
}

// Norm partials come back through pinned host memory, one double per column, written by the waves of the command that
// computes them.  The host marks every slot before it pushes that command (a NaN no computation produces) and reads a slot
// once the mark is gone: the value itself says that it has arrived -- no flag whose write would have to be ordered behind
// 832 waves' stores on their way over PCIe.
static const unsigned long long kPoison = 0x7FF8DEADBEEFCAFEull;

// the buffer the next command with partials writes to, under the controller's name for it; marked
double* nk2d_stream_part_take(nk2d_ctx* c, const double* name) {
    nk2d_stream_state* S = c->strm;
    double* buf = S->pbuf[S->pnext];
    S->pnext = (S->pnext + 1) % NK2D_PART_RING;
    int slot = -1;
    for (int i = 0; i < NK2D_PART_RING; ++i) {
        if (S->pmap[i].buf == buf) { S->pmap[i].name = nullptr; S->pmap[i].buf = nullptr; }   // (whoever held it has long read it)
        if (S->pmap[i].name == name) slot = i;
    }
    if (slot < 0)
        for (int i = 0; i < NK2D_PART_RING && slot < 0; ++i)
            if (S->pmap[i].name == nullptr) slot = i;
    S->pmap[slot].name = name;
    S->pmap[slot].buf = buf;
    unsigned long long* p = reinterpret_cast<unsigned long long*>(buf);
    for (int i = 0; i < c->ncol; ++i) __atomic_store_n(p + i, kPoison, __ATOMIC_RELAXED);
    return buf;
}

// the buffer the controller's name stands for right now (the name itself where no command has taken it)
const double* nk2d_stream_part_named(const nk2d_ctx* c, const double* name) {
    const nk2d_stream_state* S = c->strm;
    if (S)
        for (int i = 0; i < NK2D_PART_RING; ++i)
            if (S->pmap[i].name == name && S->pmap[i].buf) return S->pmap[i].buf;
    return name;
}

// a launch writes partials to the name itself: the name stands for itself again
void nk2d_stream_part_forget(nk2d_ctx* c, const double* name) {
    nk2d_stream_state* S = c->strm;
    if (!S) return;
    for (int i = 0; i < NK2D_PART_RING; ++i)
        if (S->pmap[i].name == name || name == nullptr) { S->pmap[i].name = nullptr; S->pmap[i].buf = nullptr; }   // (null: every name)
}

int nk2d_stream_wait_part(nk2d_ctx* c, const double* name, int n) {
    nk2d_stream_state* S = c->strm;
    if (!S || S->lost) return NK2D_RC_STREAM_LOST;
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(nk2d_stream_part_named(c, name));
    const auto t0 = std::chrono::steady_clock::now();
    const double limit_s = 1.0e-3 * c->barrier_timeout_ms + 1.0;
    long long spins = 0;
    for (int i = 0; i < n; ++i) {
        while (__atomic_load_n(p + i, __ATOMIC_ACQUIRE) == kPoison) {
            if ((++spins & 255) == 0) {
                const bool gave_up = __atomic_load_n(S->h_status, __ATOMIC_RELAXED) != 0;
                const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (gave_up || waited > limit_s) {
                    S->lost = true;
                    c->stream_timeouts++;
                    (void)nk2d_stream_pause(c);
                    (void)hipStreamSynchronize(c->stream_);
                    return NK2D_RC_STREAM_LOST;
                }
            }
        }
    }
    return 0;
}

int nk2d_stream_push(nk2d_ctx* c, StreamCmd& cmd, bool notify, unsigned* seq_out) {
    if (c->tape_rec) {
        // recording a tape (option "frozen_tape"): the command goes to the tape, packed; nothing runs, nothing is counted.
        // A command behind the year's last commit (a launch, after the tape) would run out of order: the tape is refused.
        nk2d_tape* T = c->tape;
        if (T->fin_out) c->tape_foreign++;
        unsigned dw[NK2D_CMD_DWORDS] = {0};
        cmd.flags &= ~NK2D_CMD_NOTIFY;
        std::memcpy(dw, &cmd, sizeof(StreamCmd));
        const int ndw = cmd_dwords(cmd.op);
        dw[0] = (unsigned)cmd.op | ((unsigned)ndw << 16);
        T->cmds.insert(T->cmds.end(), dw, dw + ndw);
        T->ncmd++;
        if (seq_out) *seq_out = 0;
        return 0;
    }
    NK2D_TRY(stream_alloc(c));
    nk2d_stream_state* S = c->strm;
    if (S->lost) return NK2D_RC_STREAM_LOST;
    if (!S->running) NK2D_TRY(stream_start(c));
    const unsigned seq = S->seq + 1;
    // flow control: a slot is rewritten NK2D_RING_SLOTS commands later -- by then every workgroup must be past it.  Every
    // 32nd command asks for completion stamps; the host never runs more than half a ring ahead of the oldest of them
    if ((seq & 31u) == 0) notify = true;
    while (seq - S->done_upto > NK2D_RING_SLOTS / 2 && !S->notifies.empty()) NK2D_TRY(nk2d_stream_wait(c, S->notifies.front()));
    cmd.flags = (cmd.flags & ~NK2D_CMD_NOTIFY) | (notify ? NK2D_CMD_NOTIFY : 0);
    ring_write(S, seq, cmd);
    S->seq = seq;
    if (notify) S->notifies.push_back(seq);
    if (seq_out) *seq_out = seq;
    c->stream_cmds++;
    return 0;
}

// tell the kernel to finish behind the commands pushed so far; nothing is waited for (what the caller queues on the
// context's stream next is ordered behind the kernel by the stream)
int nk2d_stream_pause(nk2d_ctx* c) {
    nk2d_stream_state* S = c->strm;
    if (!S || !S->running) return 0;
    StreamCmd cmd = {};
    cmd.op = NK2D_OP_EXIT;
    const unsigned seq = S->seq + 1;
    ring_write(S, seq, cmd);
    S->seq = seq;
    S->running = false;
    // (the kernel's workgroups all pass the EXIT command: everything before it is complete once the kernel has ended)
    S->notifies.clear();
    nk2d_turn_give(S->turn_waves);
    return 0;
}

// the end of a year: the kernel ends, the host waits for it and learns whether it had given up on the way
int nk2d_stream_end(nk2d_ctx* c) {
    nk2d_stream_state* S = c->strm;
    if (!S) return 0;
    (void)nk2d_stream_pause(c);
    NK2D_CHECK(c, hipMemcpyAsync(S->h_out, S->d_out, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream_));
    NK2D_CHECK(c, hipStreamSynchronize(c->stream_));
    S->done_upto = S->seq;
    const bool lost = S->lost || S->h_out[0] != 0.0 || __atomic_load_n(S->h_status, __ATOMIC_RELAXED) != 0;
    if (lost) {
        // leave everything as a fresh start would find it
        if (!S->lost) c->stream_timeouts++;
        S->lost = false;
        std::memset(S->h_status, 0, sizeof(unsigned) * 16);
        NK2D_CHECK(c, hipMemset(S->d_sync, 0, 4096));
        NK2D_CHECK(c, hipMemset(S->d_out, 0, sizeof(double) * 8));
        return NK2D_RC_STREAM_LOST;
    }
    return 0;
}

// where the workgroups' time went since the context was created: microseconds per workgroup (mean over the workgroups)
// waiting for commands, executing them, waiting for the lateral neighbours; commands per workgroup
// out[12]: 0..2 as above, 3 commands, 4..7 microseconds executing SETUP / NEWTON / ERR / BOUNDARY commands, 8..11 their counts
int nk2d_stream_profile(nk2d_ctx* c, double* out12) {
    nk2d_stream_state* S = c->strm;
    for (int i = 0; i < 12; ++i) out12[i] = 0.0;
    if (!S) return 0;
    std::vector<unsigned long long> h((size_t)12 * S->nwg);
    NK2D_CHECK(c, hipMemcpy(h.data(), S->d_prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    for (int wg = 0; wg < S->nwg; ++wg)
        for (int i = 0; i < 12; ++i) out12[i] += (double)h[(size_t)12 * wg + i];
    for (int i = 0; i < 12; ++i) out12[i] *= ((i < 3 || (i >= 4 && i < 8)) ? 0.01 : 1.0) / S->nwg;      // ticks of 10 ns -> us
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the tape (option "frozen_tape", nk2d_stream.h)
// ---------------------------------------------------------------------------------------------------------------------
// the recorded commands, EXIT appended, into HBM (once per schedule; the allocation is kept and grows)
int nk2d_tape_upload(nk2d_ctx* c, nk2d_tape* T) {
    const unsigned exit_dw = (unsigned)NK2D_OP_EXIT | ((unsigned)cmd_dwords(NK2D_OP_EXIT) << 16);
    T->cmds.push_back(exit_dw);
    for (int k = 1; k < cmd_dwords(NK2D_OP_EXIT); ++k) T->cmds.push_back(0u);
    T->ncmd++;
    const size_t need = T->cmds.size();
    if (T->dev_dwords < need) {
        NK2D_CHECK(c, hipStreamSynchronize(nk2d_s(c)));
        if (T->dev) NK2D_CHECK(c, hipFree(T->dev));
        T->dev = nullptr;
        T->dev_dwords = 0;
        NK2D_CHECK(c, hipMalloc((void**)&T->dev, sizeof(unsigned) * need));
        T->dev_dwords = need;
    }
    NK2D_CHECK(c, hipMemcpyAsync(T->dev, T->cmds.data(), sizeof(unsigned) * need, hipMemcpyHostToDevice, nk2d_s(c)));
    return 0;
}

void nk2d_tape_forget(nk2d_ctx* c) {
    if (c->tape) c->tape->key = 0;
}

int64_t nk2d_tape_size(const nk2d_ctx* c, int what) {
    const nk2d_tape* T = c->tape;
    if (!T || !T->key) return 0;
    return what == 0 ? (int64_t)(sizeof(unsigned) * T->cmds.size()) : T->ncmd;
}

// The whole frozen year as ONE launch of the tape flavour of the resident kernel, on the shape of the context's command
// stream (its workgroups, columns per workgroup, LDS copies, one or two waves to a SIMD).  The host waits for the end of the
// kernel only: NK2D_RC_STREAM_LOST when a workgroup gave up on a wait (the caller reruns the year by the existing path),
// 1 when the tape flavour cannot have every workgroup resident (nothing has run).
int nk2d_tape_run(nk2d_ctx* c, nk2d_tape* T) {
    NK2D_TRY(stream_alloc(c));
    nk2d_stream_state* S = c->strm;
    (void)nk2d_s(c);      // (a host-fed kernel still running ends first)
    DevP P = make_devp(c);
    StreamArgs A = {};
    const size_t lds = stream_lds_bytes(c, S->cpw, S->coef_lds);
    {
        hipDeviceProp_t prop;
        NK2D_CHECK(c, hipGetDeviceProperties(&prop, c->dev));
        int per_cu = 0;
        NK2D_CHECK(c, stream_launch(c, dim3(1), dim3(64 * S->nw), P, A, &per_cu, lds, S->two_waves, true));
        if (per_cu * prop.multiProcessorCount < S->nwg) return 1;
    }
    A.abort_flag = (int*)S->d_sync;
    A.flags = (unsigned*)(S->d_sync + 4096);
    A.h_status = S->h_status; A.out = S->d_out;
    A.seq0 = S->seq + 1;
    A.nwg = S->nwg; A.cpw = S->cpw;
    A.spin_ticks = (long long)(c->barrier_timeout_ms * 1.0e5);
    A.fences = c->year_fences;
    A.prof = S->d_prof;
    A.coef_lds = S->coef_lds ? 3 : 0;
    A.W = c->W;
    A.tape = T->dev;
    A.tape_dwords = T->cmds.size();
    const int waves = S->nwg * S->nw;
    nk2d_turn_take(waves);
    const hipError_t rc = stream_launch(c, dim3(S->nwg), dim3(64 * S->nw), P, A, nullptr, lds, S->two_waves, true);
    if (rc != hipSuccess) {
        nk2d_turn_give(waves);
        NK2D_CHECK(c, rc);
    }
    c->stream_xlane_bits = 0;      // (the tape flavour has today's body only)
    // (the stamps of the workgroups' flags go on from here: a host-fed kernel after this one starts behind the EXIT)
    S->seq += (unsigned)T->ncmd;
    S->done_upto = S->seq;
    const hipError_t c1 = hipMemcpyAsync(S->h_out, S->d_out, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream_);
    const hipError_t c2 = (c1 == hipSuccess) ? hipStreamSynchronize(c->stream_) : c1;
    nk2d_turn_give(waves);
    NK2D_CHECK(c, c2);
    c->st.nlaunch++;
    if (S->h_out[0] != 0.0 || __atomic_load_n(S->h_status, __ATOMIC_RELAXED) != 0) {
        std::memset(S->h_status, 0, sizeof(unsigned) * 16);
        NK2D_CHECK(c, hipMemset(S->d_sync, 0, 4096));
        NK2D_CHECK(c, hipMemset(S->d_out, 0, sizeof(double) * 8));
        return NK2D_RC_STREAM_LOST;
    }
    return 0;
}
