// frt_refit_device.hip — kernels of frt_renderer_set_instance_transforms_ex with FRT_TRANSFORM_DEVICE ("Transforms from device memory";
// frt_refit_device.hpp). Built with the library's contract flags (-ffp-contract=off, no fast math, IEEE division and square root): the arithmetic is
// frt_instance_record.hpp's and frt_refit.hpp's, operation by operation what the host form computes, and no fma is written by hand.
// Visibility between the launches comes from kernel boundaries on one stream, as everywhere in the refit: what one launch writes (the flag, `last`, the
// matrix table) the next reads. One thread per record or triangle, consecutive threads on consecutive elements, vector loads and stores, no LDS.
#include "frt_refit_device.hpp"
#include "frt_instance_record.hpp"

namespace frt {

static const int kXformBlock = 256;
static const uint32_t kXformNone = 0xFFFFFFFFu;

__device__ inline void load_matrix(const float4* q, float m[16]) {
    for (int c = 0; c < 4; ++c) { const float4 v = q[c]; m[4 * c] = v.x; m[4 * c + 1] = v.y; m[4 * c + 2] = v.z; m[4 * c + 3] = v.w; }
}

// Thread k: record k of the call.
__global__ void __launch_bounds__(kXformBlock) transform_validate_kernel(TransformInput a) {
    const uint32_t k = blockIdx.x * (uint32_t)kXformBlock + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t id = a.ids[k];
    float m[16], w2o[9];
    uint32_t flip;
    load_matrix(a.mats + 4u * (size_t)k, m);
    if (id >= a.num_inst || !record_instance_inverse(m, w2o, flip)) { atomicOr(a.reject, 1u); return; }
    atomicMax(a.last + id, k + 1u);
}

// Thread k: record k; it writes when it is the last record of its instance (what an id given twice ends with).
__global__ void __launch_bounds__(kXformBlock) transform_records_kernel(SceneView sc, TransformInput a) {
    const uint32_t k = blockIdx.x * (uint32_t)kXformBlock + threadIdx.x;
    if (k >= a.n) return;
    if (a.reject[0]) { if (k == 0u) atomicAdd(a.reject + 1, 1u); return; }
    const uint32_t id = a.ids[k];
    if (id >= a.num_inst || a.last[id] != k + 1u) return;
    const float4* src = a.mats + 4u * (size_t)k;
    float m[16];
    load_matrix(src, m);
    for (int c = 0; c < 4; ++c) a.m[4u * (size_t)id + (uint32_t)c] = src[c];
    const InstanceConst& ic = a.consts[id];
    InstanceView d;
    d.mesh_id = ic.mesh_id; d.mat_id = ic.mat_id; d.first_tri = ic.first_tri; d.flip = 0u;
    for (int i = 0; i < 9; ++i) d.w2o[i] = 0.0f;
    d.pad[0] = d.pad[1] = d.pad[2] = 0.0f;
    record_instance_inverse(m, d.w2o, d.flip);
    const_cast<InstanceView*>(sc.instances)[id] = d;
    if (ic.light == kXformNone || ic.light >= sc.num_lights) return;
    const LightRecord l = ic.light_kind == 0u ? record_quad_light(m, ic.emission) : record_sphere_light(m, ic.emission);
    float4* out = reinterpret_cast<float4*>(const_cast<LightView*>(sc.lights) + ic.light);
    out[0] = make_float4(l.position[0], l.position[1], l.position[2], __uint_as_float(l.type_));
    out[1] = make_float4(l.u[0], l.u[1], l.u[2], l.area);
    out[2] = make_float4(l.v[0], l.v[1], l.v[2], __uint_as_float(l.pad));
    out[3] = make_float4(l.emission[0], l.emission[1], l.emission[2], l.emission[3]);
}

// Thread g: flattened triangle g of the scene. Its instance is the one its slot names; it is rewritten when that instance moved in this call.
__global__ void __launch_bounds__(kXformBlock) transform_triangles_kernel(SceneView sc, TransformInput a) {
    const uint32_t g = blockIdx.x * (uint32_t)kXformBlock + threadIdx.x;
    if (g >= sc.num_tris) return;
    if (a.reject[0]) return;
    const uint32_t slot = a.slot_of[g];
    if (slot >= sc.num_tris) return;
    const uint32_t inst = __float_as_uint(sc.tris[3u * (size_t)slot + 1u].w);
    if (inst >= a.num_inst || a.last[inst] == 0u) return;
    const float4 head = reinterpret_cast<const float4*>(a.consts + inst)[0];      // (first_tri, tri_count, index_offset, pos_offset)
    const uint32_t first_tri = __float_as_uint(head.x), tri_count = __float_as_uint(head.y), index_offset = __float_as_uint(head.z), pos_offset = __float_as_uint(head.w);
    if (g < first_tri || g - first_tri >= tri_count) return;
    const uint32_t j = g - first_tri;
    if ((uint64_t)index_offset + 3ull * j + 2ull >= a.cap_indices) return;
    float m[12];
    for (int c = 0; c < 4; ++c) { const float4 v = a.m[4u * (size_t)inst + (uint32_t)c]; m[3 * c] = v.x; m[3 * c + 1] = v.y; m[3 * c + 2] = v.z; }
    float4 p[3];
    float w[3][3];
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = sc.indices[index_offset + 3u * j + (uint32_t)k];
        if ((uint64_t)pos_offset + v >= a.cap_verts) return;
        p[k] = a.pos[pos_offset + v];
    }
    instance_world_vertices(m, p, w);
    store_tri_slot(const_cast<float4*>(sc.tris) + (size_t)slot * 3u, w, g, inst);
}

hipError_t launch_device_transforms(const SceneView& sc, const TransformInput& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.reject, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (a.num_inst && (e = hipMemsetAsync(a.last, 0, (size_t)a.num_inst * sizeof(uint32_t), stream)) != hipSuccess) return e;
    const dim3 rec_grid((a.n + kXformBlock - 1) / kXformBlock);
    hipLaunchKernelGGL(transform_validate_kernel, rec_grid, dim3(kXformBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(transform_records_kernel, rec_grid, dim3(kXformBlock), 0, stream, sc, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (sc.num_tris > 0) hipLaunchKernelGGL(transform_triangles_kernel, dim3((sc.num_tris + kXformBlock - 1) / kXformBlock), dim3(kXformBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
