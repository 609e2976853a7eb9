// frt_deform.hip — kernel of frt_renderer_set_mesh_vertices ("Deforming meshes"; frt_deform.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math): the transform is world_triangle's (frt_scene.cpp) operation by
// operation and no fma is written by hand. The shading record is a gather: every word of it is copied from the uploaded attributes, from the
// host-decoded vertex normals or from the record it replaces (the material word), so it equals build_gpu_layout's record bit for bit.
// Visibility: the copies that bring the new vertices precede the kernel on its stream, the extent pass and the refit follow it there.
#include "frt_deform.hpp"

namespace frt {

static const int kDeformBlock = 256;

// Thread g: triangle g - work_begin of the record that holds g (a binary search over the prefix sums, as instance_transform_kernel's).
__global__ void __launch_bounds__(kDeformBlock) mesh_deform_kernel(SceneView sc, DeformArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    if (g >= a.work) return;
    uint32_t lo = 0, hi = a.nrec;      // the last record with work_begin <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.rec[mid].work_begin <= g) lo = mid; else hi = mid; }
    const float4* rq = reinterpret_cast<const float4*>(a.rec + lo);      // 64 B: (id, first_tri, tri_count, work_begin) and m[12]
    const float4 head = rq[0], m0 = rq[1], m1 = rq[2], m2 = rq[3];
    const uint32_t inst = __float_as_uint(head.x), first_tri = __float_as_uint(head.y), tri_count = __float_as_uint(head.z);
    const uint32_t j = g - __float_as_uint(head.w);
    if (j >= tri_count) return;
    const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
    uint32_t v[3];
    float4 p[3];
    float w[3][3];
    for (int k = 0; k < 3; ++k) { v[k] = sc.indices[a.index_offset + 3u * j + (uint32_t)k]; p[k] = a.pos[a.pos_offset + v[k]]; }
    instance_world_vertices(m, p, w);
    const uint32_t id = first_tri + j;
    if (id >= sc.num_tris) return;
    const uint32_t slot = a.slot_of[id];
    if (slot >= sc.num_tris) return;
    store_tri_slot(const_cast<float4*>(sc.tris) + (size_t)slot * 3u, w, id, inst);
    if (!a.normals) return;
    // shading record (frt_deform.hpp: store_shade_corners); the material word and what follows it stay
    const float4* at = reinterpret_cast<const float4*>(sc.attributes + a.attr_offset);      // per vertex: (normal.xy, uv.xy) (tangent.xyzw)
    float4 n[3], nu[3], tg[3];
    for (int k = 0; k < 3; ++k) { n[k] = a.normals[v[k]]; nu[k] = at[2u * v[k]]; tg[k] = at[2u * v[k] + 1u]; }
    float4* rec = const_cast<float4*>(sc.shade_tris) + (size_t)id * 8u;
    const float4 old6 = rec[6];
    store_shade_corners(rec, n, nu, tg);
    rec[6] = make_float4(tg[0].w, old6.y, old6.z, old6.w);
}

hipError_t launch_mesh_deform(const SceneView& sc, const DeformArgs& a, hipStream_t stream) {
    if (a.work == 0 || a.nrec == 0) return hipSuccess;
    hipLaunchKernelGGL(mesh_deform_kernel, dim3((a.work + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
