// nk2d_frozen_d.hip -- the one-launch frozen year's kernel (nk2d_frozen.hip, nk2d_frozen_body.inc) with the body of the default year
// alone: k_frozen_persistent carries twenty Newton bodies (ten sets of what lives in LDS and registers, each with and without the
// step's end) and picks one at run time; a year with every option at its default runs CL 959 and nothing else.  Here the same
// text is compiled with FZ_ONLY 959: that one body, and what the host guarantees for it as constants.  The device functions and
// their template arguments are k_frozen_persistent's: the same year, bit for bit.  Option "frozen_dedicated" (frozen_dedicated(),
// nk2d_frozen_plan.h) routes a year here; bit 11 of A.coef_lds picks the hand-over's poll (NeighbourSync::wait_one_load()).
// A unit of its own so that these instantiations compile beside k_frozen_persistent's, which stay the functions they are.
#include "nk2d_bodies.h"
#include "nk2d_frozen_plan.h"

template <int E, int KIND, int PIECES>
__global__ void __launch_bounds__(NK2D_BLOCK) k_frozen_persistent_d(DevP P, typename FrozenArgOf<PIECES>::type A) {
    constexpr int TEAM = 0, LEAN = 0;
#define FZ_ONLY 959
#include "nk2d_frozen_body.inc"
#undef FZ_ONLY
}

template <int E, int KIND, int PIECES>
static hipError_t frozen_launch_d_one(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, typename FrozenArgOf<PIECES>::type& A, int* max_blocks,
                                      size_t lds_bytes) {
    if constexpr (NK2D_FROZEN_DEDICATED(E, KIND, PIECES)) {
        if (max_blocks) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, k_frozen_persistent_d<E, KIND, PIECES>, (int)block.x, lds_bytes);
        hipLaunchKernelGGL((k_frozen_persistent_d<E, KIND, PIECES>), grid, block, lds_bytes, nk2d_s(c), P, A);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

template <int E, int KIND>
static hipError_t frozen_launch_d_ek(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, FrozenPieceArgs& A, bool pieces, int* max_blocks, size_t lds_bytes) {
    if (pieces) return frozen_launch_d_one<E, KIND, 1>(c, grid, block, P, A, max_blocks, lds_bytes);
    return frozen_launch_d_one<E, KIND, 0>(c, grid, block, P, static_cast<FrozenArgs&>(A), max_blocks, lds_bytes);
}

// max_blocks: nothing is launched, the answer is the kernel's occupancy (workgroups of `block` with `lds_bytes` per compute unit)
hipError_t nk2d_frozen_launch_d(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, FrozenPieceArgs& A, bool pieces, int* max_blocks, size_t lds_bytes) {
    const bool forced = c->kind == 2;
    if (c->kind != 0 && !forced) return hipErrorInvalidValue;
    switch (c->E) {
        case 5: return forced ? frozen_launch_d_ek<5, 2>(c, grid, block, P, A, pieces, max_blocks, lds_bytes)
                              : frozen_launch_d_ek<5, 0>(c, grid, block, P, A, pieces, max_blocks, lds_bytes);
        case 6: return forced ? frozen_launch_d_ek<6, 2>(c, grid, block, P, A, pieces, max_blocks, lds_bytes)
                              : frozen_launch_d_ek<6, 0>(c, grid, block, P, A, pieces, max_blocks, lds_bytes);
        case 7: return forced ? frozen_launch_d_ek<7, 2>(c, grid, block, P, A, pieces, max_blocks, lds_bytes)
                              : frozen_launch_d_ek<7, 0>(c, grid, block, P, A, pieces, max_blocks, lds_bytes);
        default: break;
    }
    return hipErrorInvalidValue;
}
