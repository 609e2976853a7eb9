// frt_skin.hip — kernel of frt_renderer_set_mesh_pose ("Skinning"; frt_skin.hpp). Built with the library's contract flags
// (-ffp-contract=off, no fast math): the vertex is frt_skin.hpp's skinned_position, the function the host specification calls. A translation unit of its
// own: it includes none of the frame kernels' headers beyond frt_math.hpp.
#include "frt_skin.hpp"

namespace frt {

static const int kSkinBlock = 256;

__device__ inline bool skin_finite4(float4 q) {
    return ((__float_as_uint(q.x) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.y) & 0x7f800000u) != 0x7f800000u) &&
           ((__float_as_uint(q.z) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.w) & 0x7f800000u) != 0x7f800000u);
}

__global__ void __launch_bounds__(kSkinBlock) mesh_skin_kernel(SkinArgs a) {
    const uint32_t v = blockIdx.x * (uint32_t)kSkinBlock + threadIdx.x;
    // (every thread that raises the flag stores the same word: a plain store, no atomic)
    if (a.check_palette && v < 4u * a.njoints && !skin_finite4(a.palette[v])) a.reject[0] = 1u;
    if (v >= a.nverts || v >= a.out_len) return;
    const float4 p = a.bind[v], wt = a.weights[v];
    const uint2 jw = a.joints[v];
    const uint32_t j[4] = {jw.x & 0xFFFFu, jw.x >> 16, jw.y & 0xFFFFu, jw.y >> 16};
    if (j[0] >= a.njoints || j[1] >= a.njoints || j[2] >= a.njoints || j[3] >= a.njoints) { a.reject[0] = 1u; return; }
    float m[4][16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4* c = a.palette + 4u * (size_t)j[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 q = c[i]; m[k][4 * i] = q.x; m[k][4 * i + 1] = q.y; m[k][4 * i + 2] = q.z; m[k][4 * i + 3] = q.w; }
    }
    const float pb[4] = {p.x, p.y, p.z, p.w}, w[4] = {wt.x, wt.y, wt.z, wt.w};
    float o[4];
    skinned_position(pb, m, w, o);
    a.out[v] = make_float4(o[0], o[1], o[2], o[3]);
}

hipError_t launch_mesh_skin(const SkinArgs& a, hipStream_t stream) {
    if (a.nverts == 0) return hipSuccess;
    if (a.njoints == 0 || a.njoints > 0x10000u) return hipErrorInvalidValue;      // (a joint index is 16 bits)
    const uint32_t threads = a.check_palette && 4u * a.njoints > a.nverts ? 4u * a.njoints : a.nverts;
    hipLaunchKernelGGL(mesh_skin_kernel, dim3((threads + kSkinBlock - 1) / kSkinBlock), dim3(kSkinBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace frt
