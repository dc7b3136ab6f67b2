// nk2d_stream_xl.hip -- the command-stream kernel (nk2d_stream.h, nk2d_stream_body.inc) in the flavour of option "stream_xlane":
// every command's cross-lane moves at distances 1 and 32, and its wave sums, in the VALU (the xl_ helpers of nk2d_common.h,
// NK2D_FROZEN_XLANE_MOVES) instead of ds_bpermute.  The host-fed kernel only, in the classes NK2D_STREAM_XLANE names; a unit of its
// own so that these instantiations compile beside today's (nk2d_stream.hip), which stay the functions they are.
#include "nk2d_stream.h"

#include "nk2d_stream_body.inc"

template <int E, int KIND>
static hipError_t stream_launch_one_xl(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, StreamArgs& A, int* max_blocks, size_t lds_bytes,
                                       bool two_waves) {
    constexpr int XL = NK2D_FROZEN_XLANE_MOVES;
    if constexpr (kStreamHasTwoWaves<E, KIND>) {
        if (two_waves) {
            if constexpr (NK2D_STREAM_XLANE(E, KIND, 1)) {
                if (max_blocks)
                    return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, k_stream_w2<E, KIND, false, XL>, (int)block.x, lds_bytes);
                hipLaunchKernelGGL((k_stream_w2<E, KIND, false, XL>), grid, block, lds_bytes, c->stream_, P, A);
                return hipGetLastError();
            } else {
                return hipErrorInvalidValue;
            }
        }
    } else if (two_waves) {
        return hipErrorInvalidValue;
    }
    if constexpr (NK2D_STREAM_XLANE(E, KIND, 0)) {
        if (max_blocks) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, k_stream<E, KIND, false, XL>, (int)block.x, lds_bytes);
        hipLaunchKernelGGL((k_stream<E, KIND, false, XL>), grid, block, lds_bytes, c->stream_, P, A);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

hipError_t nk2d_stream_launch_xl(nk2d_ctx* c, dim3 grid, dim3 block, DevP& P, StreamArgs& A, int* max_blocks, size_t lds_bytes, bool two_waves) {
    hipError_t rc = hipErrorInvalidValue;
    NK2D_DISPATCH_EK(c->E, c->kind, rc = (stream_launch_one_xl<EE, KK>(c, grid, block, P, A, max_blocks, lds_bytes, two_waves)));
    return rc;
}
