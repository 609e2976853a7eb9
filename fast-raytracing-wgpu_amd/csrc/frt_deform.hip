// frt_deform.hip — kernel of frt_renderer_set_mesh_vertices ("Deforming meshes"; frt_deform.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math): the transform is world_triangle's (frt_scene.cpp) operation by
// operation and no fma is written by hand. The shading record is a gather: every word of it is copied from the uploaded attributes, from the
// host-decoded vertex normals or from the record it replaces (the material word), so it equals build_gpu_layout's record bit for bit.
// Visibility: the copies that bring the new vertices precede the kernel on its stream, the extent pass and the refit follow it there.
//
// The normal pass and the device-input kernels (frt_deform.hpp) follow the same rules. The normal of a vertex is frt_vertex_normal.hpp's
// recomputed_vertex_normal, the function the host specification calls, compiled here under the same flags: IEEE +, -, *, /, sqrt in the same order.
// Of the two designs that give these bits — recompute the triangle's cross product at every corner that gathers it, or write it once per triangle into
// scratch and gather that — the product runs the first: no scratch, one launch. The second is compiled into lib/libfrt_exp.so only, where it was measured
// against the first ("Recomputed normals").
#include "frt_deform.hpp"
#include "frt_vertex_normal.hpp"

namespace frt {

static const int kDeformBlock = 256;

// Thread g: triangle g - work_begin of the record that holds g (a binary search over the prefix sums, as instance_transform_kernel's).
__global__ void __launch_bounds__(kDeformBlock) mesh_deform_kernel(SceneView sc, DeformArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    if (g >= a.work) return;
    if (a.reject && *a.reject) return;      // a rejected device-input call: nothing is applied
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

// ------------------------------------------------------------------------------------------------ recomputed normals
__global__ void __launch_bounds__(kDeformBlock) vertex_normal_kernel(SceneView sc, NormalArgs a) {
    const uint32_t v = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    if (v >= a.nverts) return;
    if (a.reject && *a.reject) return;
    const uint32_t dst = a.attr_offset + v;
    if (dst >= a.cap_verts) return;      // (that the mesh's positions and indices lie inside their pools is the host's check, once per call, in 64 bits)
    const uint32_t begin = a.adj_offsets[v], end = a.adj_offsets[v + 1u];
    float4* at = reinterpret_cast<float4*>(const_cast<VertexAttrView*>(sc.attributes)) + 2u * (size_t)dst;
    float4 nu = at[0];
    f2 e;
    bool fresh = false;
    if (begin <= end && end <= a.nidx) {
#if defined(FRT_EXPERIMENTS) && FRT_EXPERIMENTS
        if (a.tri_scratch) {
            f3 s = mk3(0.0f, 0.0f, 0.0f);
            for (uint32_t c = begin; c < end; ++c) {
                const uint32_t j = a.adj_corners[c] / 3u;
                if (j >= a.nidx / 3u) continue;
                const float4 q = a.tri_scratch[j];
                s = s + mk3(q.x, q.y, q.z);
            }
            fresh = finish_vertex_normal(s, begin < end, e);
        } else
#endif
        fresh = recomputed_vertex_normal(a.adj_corners, begin, end, sc.indices + a.index_offset, a.nidx, a.pos + a.pos_offset, a.nverts, e);
    }
    if (fresh) {
        *reinterpret_cast<float2*>(at) = make_float2(e.x, e.y);
        nu.x = e.x; nu.y = e.y;
    }
    const f3 n = decode_octahedral_normal(nu.x, nu.y);      // of what the attribute holds now, as the host decodes it
    const float4 dn = make_float4(n.x, n.y, n.z, 0.0f);
    a.block[v] = dn;
    if (a.pool_normals) a.pool_normals[dst] = dn;
}

#if defined(FRT_EXPERIMENTS) && FRT_EXPERIMENTS
// Thread j: the normal of triangle j of the mesh into the scratch (an index out of range, which no mesh holds: zero).
__global__ void __launch_bounds__(kDeformBlock) triangle_normal_kernel(SceneView sc, NormalArgs a) {
    const uint32_t j = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    if (j >= a.nidx / 3u) return;
    if (a.reject && *a.reject) return;
    const uint32_t* idx = sc.indices + a.index_offset + 3u * (size_t)j;
    const uint32_t i0 = idx[0], i1 = idx[1], i2 = idx[2];
    f3 c = mk3(0.0f, 0.0f, 0.0f);
    if (i0 < a.nverts && i1 < a.nverts && i2 < a.nverts) {
        const float4 p = a.pos[a.pos_offset + i0], q = a.pos[a.pos_offset + i1], w = a.pos[a.pos_offset + i2];
        c = triangle_area_normal(mk3(p.x, p.y, p.z), mk3(q.x, q.y, q.z), mk3(w.x, w.y, w.z));
    }
    a.tri_scratch[j] = make_float4(c.x, c.y, c.z, 0.0f);
}
#endif

hipError_t launch_vertex_normals(const SceneView& sc, const NormalArgs& a, hipStream_t stream) {
    if (a.nverts == 0) return hipSuccess;
#if defined(FRT_EXPERIMENTS) && FRT_EXPERIMENTS
    if (a.tri_scratch && a.nidx >= 3u) {
        hipLaunchKernelGGL(triangle_normal_kernel, dim3((a.nidx / 3u + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, sc, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
#endif
    hipLaunchKernelGGL(vertex_normal_kernel, dim3((a.nverts + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, sc, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ device input
__device__ inline bool finite4(float4 q) {
    return ((__float_as_uint(q.x) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.y) & 0x7f800000u) != 0x7f800000u) &&
           ((__float_as_uint(q.z) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.w) & 0x7f800000u) != 0x7f800000u);
}
// Thread g: float4 g of the positions, then of the attributes.
__global__ void __launch_bounds__(kDeformBlock) deform_validate_kernel(DeformInput a) {
    const uint32_t g = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    const uint32_t words = a.attrs ? 3u * a.nverts : a.nverts;
    if (g >= words) return;
    const float4 q = g < a.nverts ? a.pos[g] : a.attrs[g - a.nverts];
    if (!finite4(q)) atomicOr(a.reject, 1u);
}
__global__ void __launch_bounds__(kDeformBlock) deform_copy_in_kernel(DeformInput a) {
    const uint32_t v = blockIdx.x * (uint32_t)kDeformBlock + threadIdx.x;
    if (v >= a.nverts) return;
    if (a.reject[0]) { if (v == 0u) atomicAdd(a.reject + 1, 1u); return; }
    const uint32_t dp = a.pos_offset + v, da = a.attr_offset + v;
    if (dp >= a.cap_verts || da >= a.cap_verts) return;
    a.out_pos[dp] = a.pos[v];
    if (!a.attrs) return;
    const float4 nu = a.attrs[2u * (size_t)v], tg = a.attrs[2u * (size_t)v + 1u];
    a.out_attrs[2u * (size_t)da] = nu;
    a.out_attrs[2u * (size_t)da + 1u] = tg;
    if (!a.block) return;
    const f3 n = decode_octahedral_normal(nu.x, nu.y);
    const float4 dn = make_float4(n.x, n.y, n.z, 0.0f);
    a.block[v] = dn;
    if (a.pool_normals) a.pool_normals[da] = dn;
}

hipError_t launch_deform_input(const DeformInput& a, hipStream_t stream) {
    if (a.nverts == 0 || a.nverts > 0x55555500u) return a.nverts ? hipErrorInvalidValue : hipSuccess;      // (3 nverts work items in 32 bits)
    hipError_t e = hipMemsetAsync(a.reject, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t words = a.attrs ? 3u * a.nverts : a.nverts;
    hipLaunchKernelGGL(deform_validate_kernel, dim3((words + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(deform_copy_in_kernel, dim3((a.nverts + kDeformBlock - 1) / kDeformBlock), dim3(kDeformBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace frt
