// frt_morph.hip — kernel of frt_renderer_set_mesh_morph_weights and of the morph half of frt_renderer_set_mesh_pose_ex ("Morph targets";
// frt_morph.hpp). Built with the library's contract flags (-ffp-contract=off, no fast math): the vertex is frt_morph.hpp's morphed_position, the function
// the host specification calls. A translation unit of its own: it includes none of the frame kernels' headers beyond frt_math.hpp.
#include "frt_morph.hpp"

namespace frt {

static const int kMorphBlock = 256;

__global__ void __launch_bounds__(kMorphBlock) mesh_morph_kernel(MorphArgs a) {
    const uint32_t v = blockIdx.x * (uint32_t)kMorphBlock + threadIdx.x;
    // The loads come in front of every store of this kernel, so the weight of a target, one address for the whole wave, may be a uniform load.
    if (v < a.nverts && v < a.out_len) {
        const float4 p = a.base[v];
        const float pb[4] = {p.x, p.y, p.z, p.w};
        float o[4];
        morphed_position(pb, a.deltas + 3u * (size_t)v, 3u * (size_t)a.nverts, a.weights, a.ntargets, o);
        a.out[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
    // (every thread that raises the flag stores the same word: a plain store, no atomic)
    if (a.check_weights && v < a.ntargets && (__float_as_uint(a.weights[v]) & 0x7f800000u) == 0x7f800000u) a.reject[0] = 1u;
}

hipError_t launch_mesh_morph(const MorphArgs& a, hipStream_t stream) {
    if (a.nverts == 0) return hipSuccess;
    if (a.ntargets == 0 || a.ntargets > FRT_MAX_MORPH_TARGETS) return hipErrorInvalidValue;
    const uint32_t threads = a.check_weights && a.ntargets > a.nverts ? a.ntargets : a.nverts;
    hipLaunchKernelGGL(mesh_morph_kernel, dim3((threads + kMorphBlock - 1) / kMorphBlock), dim3(kMorphBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace frt
