// frt_pose_batch.hip — kernels of every call that poses meshes: frt_renderer_set_mesh_poses, the single-mesh calls frt_renderer_set_mesh_pose(_ex) and
// _set_mesh_morph_weights (a batch of one) and the mesh half of frt_renderer_animate_cast ("Posing several meshes"; frt_pose_batch.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math, IEEE division and square root). No arithmetic is written here: a vertex is
// frt_morph.hpp's morphed_position and frt_skin.hpp's skinned_position or (a mesh bound with FRT_SKIN_DUAL_QUATERNION) skinned_position_dq, a normal frt_vertex_normal.hpp's recomputed_vertex_normal and frt_shade.hpp's
// decode_octahedral_normal, a triangle frt_refit.hpp's instance_world_vertices — the functions the host specification and frt_deform.hip's kernels call.
// The last four kernels are frt_deform.hip's (deform_validate_kernel, deform_copy_in_kernel, vertex_normal_kernel, mesh_deform_kernel) with the mesh's
// offsets and buffers taken from the thread's segment instead of the launch arguments.
// One thread per vertex or triangle of the concatenation, consecutive threads on consecutive elements, vector loads and stores, no LDS, no fences: what a
// launch writes, the next launch on the stream reads behind the kernel boundary. The segment table holds records of 80 bytes and the search reads the
// same few records in every lane of a wave that lies inside one mesh. A segment names the palette and the weights it is posed under: a wave that holds
// vertices of several meshes may pose them under several palettes (frt_renderer_animate_cast), each lane under its own segment's.
#include "frt_pose_batch.hpp"
#include "frt_vertex_normal.hpp"
#include <algorithm>

namespace frt {

static const int kPoseBlock = 256;      // four waves of 64

// The last segment whose vert_begin (ascending: a prefix sum) is <= g.
__device__ inline PoseSegment pose_segment_of(const PoseSegment* seg, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (seg[mid].vert_begin <= g) lo = mid; else hi = mid; }
    return seg[lo];
}
__device__ inline bool pose_finite4(float4 q) {
    return ((__float_as_uint(q.x) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.y) & 0x7f800000u) != 0x7f800000u) &&
           ((__float_as_uint(q.z) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(q.w) & 0x7f800000u) != 0x7f800000u);
}

// Thread g: vertex g of the concatenation, morphed from its mesh's base into the scratch the next launch reads (`morphed` when its mesh is skinned
// afterwards, else the call's posed positions). The first check_nweights threads test one device weight each, so that a bad weight whose target moves
// nothing rejects the call as the host form refuses it. (The loads come in front of every store of this kernel.)
__global__ void __launch_bounds__(kPoseBlock) pose_batch_morph_kernel(PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (g < a.total && g < a.scratch_len) {
        const PoseSegment s = pose_segment_of(a.seg, a.nseg, g);
        const uint32_t v = g - s.vert_begin;
        if (v < s.nverts && s.morph) {
            float4* out = a.morphed && s.skin ? a.morphed : a.skinned;
            const float4 p = reinterpret_cast<const float4*>(s.morph)[v];
            const float* deltas = reinterpret_cast<const float*>(s.morph + 16u * (size_t)s.nverts);
            const float pb[4] = {p.x, p.y, p.z, p.w};
            float o[4];
            morphed_position(pb, deltas + 3u * (size_t)v, 3u * (size_t)s.nverts, s.weights, s.ntargets, o);
            out[g] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    // (every thread that raises the flag stores the same word: a plain store, no atomic)
    if (a.check_weights && g < a.check_nweights && (__float_as_uint(a.check_weights[g]) & 0x7f800000u) == 0x7f800000u) a.reject[0] = 1u;
}

// Thread g: vertex g of the concatenation, skinned from its mesh's bind pose (or from the morph launch's result) into `skinned`. The first check_cols
// threads test one float4 of a device palette each, so that a bad joint no vertex names rejects the call as the host form refuses it. A joint index
// that is not below the segment's njoints (the bind call lets none in) raises the flag instead of being followed.
__global__ void __launch_bounds__(kPoseBlock) pose_batch_skin_kernel(PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (a.check_palette && g < a.check_cols && !pose_finite4(a.check_palette[g])) a.reject[0] = 1u;
    if (g >= a.total || g >= a.scratch_len) return;
    const PoseSegment s = pose_segment_of(a.seg, a.nseg, g);
    const uint32_t v = g - s.vert_begin;
    if (v >= s.nverts || !s.skin || s.skin_mode != 0u) return;      // (a segment of another mode is the dual-quaternion launch's)
    const float4* weights = reinterpret_cast<const float4*>(s.skin + 16u * (size_t)s.nverts);
    const uint2* joints = reinterpret_cast<const uint2*>(s.skin + 32u * (size_t)s.nverts);
    const float4 p = a.morphed && s.morph ? a.morphed[g] : reinterpret_cast<const float4*>(s.skin)[v], wt = weights[v];
    const uint2 jw = joints[v];
    const uint32_t j[4] = {jw.x & 0xFFFFu, jw.x >> 16, jw.y & 0xFFFFu, jw.y >> 16};
    if (j[0] >= s.njoints || j[1] >= s.njoints || j[2] >= s.njoints || j[3] >= s.njoints) { a.reject[0] = 1u; return; }
    float m[4][16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4* c = s.palette + 4u * (size_t)j[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 q = c[i]; m[k][4 * i] = q.x; m[k][4 * i + 1] = q.y; m[k][4 * i + 2] = q.z; m[k][4 * i + 3] = q.w; }
    }
    const float pb[4] = {p.x, p.y, p.z, p.w}, w[4] = {wt.x, wt.y, wt.z, wt.w};
    float o[4];
    skinned_position(pb, m, w, o);
    a.skinned[g] = make_float4(o[0], o[1], o[2], o[3]);
}

// Thread g: vertex g of the concatenation when its segment was bound with FRT_SKIN_DUAL_QUATERNION, from the same loads into the same store as the
// kernel above. Each of the vertex's four joints is converted in the lane as its four columns arrive (skin_dq_of_joint: scale, rotation quaternion,
// dual part), so one matrix is live at a time; no converted palette is staged anywhere. The palette test is this launch's when no linear launch ran in
// front of it: launch_pose_batch leaves check_palette to exactly one of the two.
__global__ void __launch_bounds__(kPoseBlock) pose_batch_skin_dq_kernel(PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (a.check_palette && g < a.check_cols && !pose_finite4(a.check_palette[g])) a.reject[0] = 1u;
    if (g >= a.total || g >= a.scratch_len) return;
    const PoseSegment s = pose_segment_of(a.seg, a.nseg, g);
    const uint32_t v = g - s.vert_begin;
    if (v >= s.nverts || !s.skin || s.skin_mode != FRT_SKIN_DUAL_QUATERNION) return;
    const float4* weights = reinterpret_cast<const float4*>(s.skin + 16u * (size_t)s.nverts);
    const uint2* joints = reinterpret_cast<const uint2*>(s.skin + 32u * (size_t)s.nverts);
    const float4 p = a.morphed && s.morph ? a.morphed[g] : reinterpret_cast<const float4*>(s.skin)[v], wt = weights[v];
    const uint2 jw = joints[v];
    const uint32_t j[4] = {jw.x & 0xFFFFu, jw.x >> 16, jw.y & 0xFFFFu, jw.y >> 16};
    if (j[0] >= s.njoints || j[1] >= s.njoints || j[2] >= s.njoints || j[3] >= s.njoints) { a.reject[0] = 1u; return; }
    SkinDualQuat dq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4* c = s.palette + 4u * (size_t)j[k];
        float m[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 q = c[i]; m[4 * i] = q.x; m[4 * i + 1] = q.y; m[4 * i + 2] = q.z; m[4 * i + 3] = q.w; }
        dq[k] = skin_dq_of_joint(m);
    }
    const float pb[4] = {p.x, p.y, p.z, p.w}, w[4] = {wt.x, wt.y, wt.z, wt.w};
    float o[4];
    skinned_position_dq(pb, dq, w, o);
    a.skinned[g] = make_float4(o[0], o[1], o[2], o[3]);
}

// Thread g: posed vertex g of the concatenation; a non-finite float of any mesh raises the flag of the whole call.
__global__ void __launch_bounds__(kPoseBlock) pose_batch_validate_kernel(PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (g >= a.total || g >= a.scratch_len) return;
    if (!pose_finite4(a.skinned[g])) atomicOr(a.reject, 1u);
}

// Thread g: posed vertex g into its mesh's place in the object-space positions. A raised flag: nothing is copied and the first thread counts the call.
__global__ void __launch_bounds__(kPoseBlock) pose_batch_copy_in_kernel(PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (g >= a.total || g >= a.scratch_len) return;
    if (a.reject[0]) { if (g == 0u) atomicAdd(a.reject + 1, 1u); return; }
    const PoseSegment s = pose_segment_of(a.seg, a.nseg, g);
    const uint32_t v = g - s.vert_begin;
    if (v >= s.nverts) return;
    const uint32_t dp = s.pos_offset + v;
    if (dp >= a.cap_verts) return;
    a.out_pos[dp] = a.skinned[g];
}

// Thread g: the normal of vertex g of the concatenation from its own mesh's triangles (vertex_normal_kernel per segment): the encoded normal into the
// attribute unless the vertex keeps its normal, what the attribute then holds decoded into block[g] and the pool of decoded normals.
__global__ void __launch_bounds__(kPoseBlock) pose_batch_normal_kernel(SceneView sc, PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (g >= a.total) return;
    if (a.reject[0]) return;
    const PoseSegment s = pose_segment_of(a.seg, a.nseg, g);
    const uint32_t v = g - s.vert_begin;
    if (v >= s.nverts || !s.adj) return;
    const uint32_t dst = s.attr_offset + v;
    if (dst >= a.cap_verts) return;      // (that the mesh's positions and indices lie inside their pools is the host's check, once per mesh, in 64 bits)
    const uint32_t nidx = 3u * s.ntris;
    const uint32_t* adj_corners = s.adj + (s.nverts + 1u);
    const uint32_t begin = s.adj[v], end = s.adj[v + 1u];
    float4* at = reinterpret_cast<float4*>(const_cast<VertexAttrView*>(sc.attributes)) + 2u * (size_t)dst;
    float4 nu = at[0];
    f2 e;
    bool fresh = false;
    if (begin <= end && end <= nidx)
        fresh = recomputed_vertex_normal(adj_corners, begin, end, sc.indices + s.index_offset, nidx, a.out_pos + s.pos_offset, s.nverts, e);
    if (fresh) {
        *reinterpret_cast<float2*>(at) = make_float2(e.x, e.y);
        nu.x = e.x; nu.y = e.y;
    }
    const f3 n = decode_octahedral_normal(nu.x, nu.y);      // of what the attribute holds now, as the host decodes it
    const float4 dn = make_float4(n.x, n.y, n.z, 0.0f);
    a.block[g] = dn;
    if (a.pool_normals) a.pool_normals[dst] = dn;
}

// Thread g: triangle g - work_begin of the instance record that holds g (mesh_deform_kernel; the record's mesh is segment rec_seg[record]).
__global__ void __launch_bounds__(kPoseBlock) pose_batch_triangle_kernel(SceneView sc, PoseBatchArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x;
    if (g >= a.work) return;
    if (a.reject[0]) return;      // a rejected call: nothing is applied
    uint32_t lo = 0, hi = a.nrec;      // the last record with work_begin <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.rec[mid].work_begin <= g) lo = mid; else hi = mid; }
    const float4* rq = reinterpret_cast<const float4*>(a.rec + lo);      // 64 B: (id, first_tri, tri_count, work_begin) and m[12]
    const float4 head = rq[0], m0 = rq[1], m1 = rq[2], m2 = rq[3];
    const uint32_t inst = __float_as_uint(head.x), first_tri = __float_as_uint(head.y), tri_count = __float_as_uint(head.z);
    const uint32_t j = g - __float_as_uint(head.w);
    const uint32_t si = a.rec_seg[lo];
    if (j >= tri_count || si >= a.nseg) return;
    const PoseSegment s = a.seg[si];
    if (j >= s.ntris) return;
    float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
    if (a.inst_m) {      // the matrix table's columns, as transform_triangles_kernel reads them: the twelve floats the mirror would hold
        if (inst >= a.num_inst) return;
        for (int c = 0; c < 4; ++c) { const float4 q = a.inst_m[4u * (size_t)inst + (uint32_t)c]; m[3 * c] = q.x; m[3 * c + 1] = q.y; m[3 * c + 2] = q.z; }
    }
    uint32_t v[3];
    float4 p[3];
    float w[3][3];
    for (int k = 0; k < 3; ++k) {
        v[k] = sc.indices[s.index_offset + 3u * j + (uint32_t)k];
        if (v[k] >= s.nverts) return;      // (no mesh holds such an index: add_mesh checks them)
        p[k] = a.out_pos[s.pos_offset + v[k]];
    }
    instance_world_vertices(m, p, w);
    const uint32_t id = first_tri + j;
    if (id >= sc.num_tris) return;
    const uint32_t slot = a.slot_of[id];
    if (slot >= sc.num_tris) return;
    store_tri_slot(const_cast<float4*>(sc.tris) + (size_t)slot * 3u, w, id, inst);
    if (!a.block) return;
    // shading record (frt_deform.hpp: store_shade_corners); the material word and what follows it stay
    const float4* at = reinterpret_cast<const float4*>(sc.attributes + s.attr_offset);      // per vertex: (normal.xy, uv.xy) (tangent.xyzw)
    const float4* normals = a.block + s.vert_begin;
    float4 n[3], nu[3], tg[3];
    for (int k = 0; k < 3; ++k) { n[k] = normals[v[k]]; nu[k] = at[2u * v[k]]; tg[k] = at[2u * v[k] + 1u]; }
    float4* rec = const_cast<float4*>(sc.shade_tris) + (size_t)id * 8u;
    const float4 old6 = rec[6];
    store_shade_corners(rec, n, nu, tg);
    rec[6] = make_float4(tg[0].w, old6.y, old6.z, old6.w);
}

static inline dim3 pose_grid(uint32_t threads) { return dim3((threads + kPoseBlock - 1) / kPoseBlock); }

hipError_t launch_pose_batch(const SceneView& sc, const PoseBatchArgs& a, hipStream_t stream) {
    const bool morph = a.morphs != 0, skin = a.skins != 0;
    if (a.nseg == 0 || a.total == 0) return hipSuccess;
    if ((!morph && !skin) || a.skins_dq > a.skins) return hipErrorInvalidValue;
    if (a.total > 0xFFFFFF00u || a.work > 0xFFFFFF00u) return hipErrorInvalidValue;      // (the work-item index is 32 bits)
    if ((a.check_palette && !skin) || (a.check_weights && !morph)) return hipErrorInvalidValue;
    if (a.check_cols > 0xFFFFFF00u || a.check_nweights > 0xFFFFFF00u) return hipErrorInvalidValue;
    if ((morph && skin) != (a.morphed != nullptr)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.reject, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (morph) {
        hipLaunchKernelGGL(pose_batch_morph_kernel, pose_grid(a.check_weights ? std::max(a.total, a.check_nweights) : a.total), dim3(kPoseBlock), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.skins > a.skins_dq) {      // a linear skin: the launch of every call before there was a second mode
        hipLaunchKernelGGL(pose_batch_skin_kernel, pose_grid(a.check_palette ? std::max(a.total, a.check_cols) : a.total), dim3(kPoseBlock), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.skins_dq) {      // the palette test runs once per call: here only when the launch above did not
        PoseBatchArgs b = a;
        if (a.skins > a.skins_dq) { b.check_palette = nullptr; b.check_cols = 0u; }
        hipLaunchKernelGGL(pose_batch_skin_dq_kernel, pose_grid(b.check_palette ? std::max(b.total, b.check_cols) : b.total), dim3(kPoseBlock), 0, stream, b);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pose_batch_validate_kernel, pose_grid(a.total), dim3(kPoseBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(pose_batch_copy_in_kernel, pose_grid(a.total), dim3(kPoseBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.block) {
        hipLaunchKernelGGL(pose_batch_normal_kernel, pose_grid(a.total), dim3(kPoseBlock), 0, stream, sc, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.work == 0 || a.nrec == 0) return hipSuccess;
    hipLaunchKernelGGL(pose_batch_triangle_kernel, pose_grid(a.work), dim3(kPoseBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
