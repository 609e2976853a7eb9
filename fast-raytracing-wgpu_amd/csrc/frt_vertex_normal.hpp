// frt_vertex_normal.hpp — recomputed vertex normals ("Recomputed normals"): the arithmetic of SceneBuilder::set_mesh_vertices under
// FRT_DEFORM_RECOMPUTE_NORMALS, __host__ __device__ so that the host specification (frt_scene.cpp) and the device pass (frt_deform.hip) compile the
// same expressions: f32, no contraction, IEEE division and square root. Beside frt_shade.hpp's decode_octahedral_normal, which both sides decode with;
// a header of its own because none of this is code of the frame's kernels.
#pragma once
#include "frt_shade.hpp"

namespace frt {

// The encoding the geometry generators store in a vertex attribute (geometry.rs:56-76; frt_scene.cpp: geometry::encode_octahedral_normal is this
// function): divisions, where the shader's encoder above multiplies by a reciprocal.
FRT_HD f2 encode_vertex_normal(f3 n) {
    float l1 = fabsf_(n.x) + fabsf_(n.y) + fabsf_(n.z);
    float rx = 0.0f, ry = 0.0f;
    if (l1 > 0.0f) { rx = n.x / l1; ry = n.y / l1; }
    if (n.z < 0.0f) {
        float fx = (1.0f - fabsf_(ry)) * (rx >= 0.0f ? 1.0f : -1.0f);
        float fy = (1.0f - fabsf_(rx)) * (ry >= 0.0f ? 1.0f : -1.0f);
        rx = fx; ry = fy;
    }
    return mk2(rx, ry);
}
// Recomputed vertex normals ("Recomputed normals"): the contract of SceneBuilder::set_mesh_vertices under FRT_DEFORM_RECOMPUTE_NORMALS,
// compiled for the host (the specification) and for the device (frt_deform.hip) from these expressions.
// The area-weighted normal of one triangle, not normalised.
FRT_HD f3 triangle_area_normal(f3 p0, f3 p1, f3 p2) {
    const f3 e1 = mk3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), e2 = mk3(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
    return mk3(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
}
// The end of a vertex's recomputation, from the sum `s` of its corners' triangle normals: false — the vertex keeps its attribute — without a corner, or when
// |s|^2 is zero or not finite; else the encoded normal of s * (1 / sqrt(|s|^2)).
FRT_HD bool finish_vertex_normal(f3 s, bool has_corner, f2& enc) {
    const float d = (s.x * s.x + s.y * s.y) + s.z * s.z;
    if (!has_corner || d == 0.0f || (f2u(d) & 0x7f800000u) == 0x7f800000u) return false;
    const float r = rsqrt_exact(d);
    enc = encode_vertex_normal(mk3(s.x * r, s.y * r, s.z * r));
    return true;
}
// The normal of the vertex named by corners [begin, end) of the mesh's vertex -> corner adjacency (`corners`: 3 * triangle + corner, ascending per vertex),
// from the mesh's indices `idx` and its new object-space positions `pos` (xyzw): s = ((0 + c_a) + c_b) + ... in adjacency order, then
// encode_vertex_normal(s * (1 / sqrt(|s|^2))). False — the vertex keeps its attribute — without a corner, or when |s|^2 is zero or not finite. An
// adjacency entry or an index out of range (there is none in a mesh the checks let in) is skipped.
template <class Pos>
FRT_HD bool recomputed_vertex_normal(const uint32_t* corners, uint32_t begin, uint32_t end, const uint32_t* idx, uint32_t nidx, const Pos* pos, uint32_t nverts, f2& enc) {
    f3 s = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t c = begin; c < end; ++c) {
        const uint32_t t = corners[c] / 3u * 3u;
        if (t >= nidx || nidx - t < 3u) continue;
        const uint32_t i0 = idx[t], i1 = idx[t + 1u], i2 = idx[t + 2u];
        if (i0 >= nverts || i1 >= nverts || i2 >= nverts) continue;
        const Pos a = pos[i0], b = pos[i1], d = pos[i2];
        s = s + triangle_area_normal(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(d.x, d.y, d.z));
    }
    return finish_vertex_normal(s, begin < end, enc);
}

} // namespace frt
