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
    float w[3][3];
    for (int k = 0; k < 3; ++k) {
        v[k] = sc.indices[a.index_offset + 3u * j + (uint32_t)k];
        const float4 p = a.pos[a.pos_offset + v[k]];
        for (int c = 0; c < 3; ++c) w[k][c] = ((m[c] * p.x + m[3 + c] * p.y) + m[6 + c] * p.z) + m[9 + c];
    }
    const uint32_t id = first_tri + j;
    if (id >= sc.num_tris) return;
    const uint32_t slot = a.slot_of[id];
    if (slot >= sc.num_tris) return;
    float4* t = const_cast<float4*>(sc.tris) + (size_t)slot * 3u;
    t[0] = make_float4(w[0][0], w[0][1], w[0][2], __uint_as_float(id));
    t[1] = make_float4(w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2], __uint_as_float(inst));
    t[2] = make_float4(w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2], 0.0f);
    if (!a.normals) return;
    // shading record (frt_shade.hpp: fetch_hit_geometry):
    //   q0 (n0.xyz, uv0.x) q1 (n1.xyz, uv0.y) q2 (n2.xyz, uv1.x) q3 (t0.xyz, uv1.y) q4 (t1.xyz, uv2.x) q5 (t2.xyz, uv2.y) q6 (tangent_sign, mat_id, -, -)
    const float4* at = reinterpret_cast<const float4*>(sc.attributes + a.attr_offset);      // per vertex: (normal.xy, uv.xy) (tangent.xyzw)
    float4 n[3], nu[3], tg[3];
    for (int k = 0; k < 3; ++k) { n[k] = a.normals[v[k]]; nu[k] = at[2u * v[k]]; tg[k] = at[2u * v[k] + 1u]; }
    float4* rec = const_cast<float4*>(sc.shade_tris) + (size_t)id * 8u;
    const float4 old6 = rec[6];
    rec[0] = make_float4(n[0].x, n[0].y, n[0].z, nu[0].z);
    rec[1] = make_float4(n[1].x, n[1].y, n[1].z, nu[0].w);
    rec[2] = make_float4(n[2].x, n[2].y, n[2].z, nu[1].z);
    rec[3] = make_float4(tg[0].x, tg[0].y, tg[0].z, nu[1].w);
    rec[4] = make_float4(tg[1].x, tg[1].y, tg[1].z, nu[2].z);
    rec[5] = make_float4(tg[2].x, tg[2].y, tg[2].z, nu[2].w);
    rec[6] = make_float4(tg[0].w, old6.y, old6.z, old6.w);
}

hipError_t launch_mesh_deform(const SceneView& sc, const DeformArgs& a, hipStream_t stream) {
    if (a.work == 0 || a.nrec == 0) return hipSuccess;
    hipLaunchKernelGGL(mesh_deform_kernel, dim3((a.work + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
