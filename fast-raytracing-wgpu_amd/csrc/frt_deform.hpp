// frt_deform.hpp — device side of frt_renderer_set_mesh_vertices ("Deforming meshes"): after the new object-space positions (and
// attributes) of one mesh have been copied into the replica, re-transform the triangles of every instance of that mesh into their slots and, when
// attributes were given, write their shading records again. The scene-extent pass and the level-by-level refit of frt_refit.hpp follow unchanged.
// The host specification is SceneBuilder::set_mesh_vertices (frt_scene.cpp); the results are bit-identical: the same f32 operations in the same
// order, no contraction, and vertex normals decoded once per vertex on the host by the function build_gpu_layout uses.
#pragma once
#include "frt_refit.hpp"

namespace frt {

// One instance of the deformed mesh, 64 B, built on the host and copied up with the others.
struct DeformInstance {
    uint32_t id;            // instance index
    uint32_t first_tri;     // its first flattened triangle id
    uint32_t tri_count;
    uint32_t work_begin;    // prefix sum of tri_count over the records before this one
    float m[12];            // columns 0..3 of the instance's current 4x4, xyz each: m[3c + r]
};
static_assert(sizeof(DeformInstance) == 64, "DeformInstance layout");

struct DeformArgs {
    const DeformInstance* rec; uint32_t nrec, work;   // records and their summed tri_count
    uint32_t index_offset;                            // of the mesh in SceneView::indices
    uint32_t pos_offset;                              // of the mesh's first vertex in `pos`
    uint32_t attr_offset;                             // of the mesh's first vertex in SceneView::attributes
    const float4* pos;                                // object-space positions of every mesh, xyzw (already the new ones)
    const float4* normals;                            // decoded normal of every vertex of the mesh (xyz, 0), or null: shading records stay
    const uint32_t* slot_of;                          // flattened triangle id -> triangle slot
    const uint32_t* reject = nullptr;                 // a device-input call's flag word (DeformInput), or null: set, the kernel returns at once
};

// ---- Recomputed normals and device input ("Recomputed normals" and "Vertices from device memory") ----
// All three kernels below: one thread per vertex or word, consecutive threads on consecutive elements, vector loads and stores, no LDS, nothing passed
// between the blocks of a launch. They run on the renderer's main stream in this order, in front of mesh_deform_kernel; what one launch writes the
// next reads behind the kernel boundary. Every destination is checked against the vertex pool's capacity before it is stored.

// The normal pass (frt_vertex_normal.hpp: recomputed_vertex_normal, the host specification's own function). Thread v: vertex v of the mesh. It stores
// the 8-byte encoded normal into SceneView::attributes unless the vertex keeps its normal, then decodes what the attribute now holds and stores that
// into `block` (what mesh_deform_kernel reads as DeformArgs::normals) and, when there is one, into the pool of decoded normals.
struct NormalArgs {
    const uint32_t* adj_offsets;      // [nverts + 1]: the mesh's vertex -> corner adjacency (build_vertex_corners), cached per mesh by the renderer
    const uint32_t* adj_corners;      // [nidx]
    uint32_t nverts, nidx;
    uint32_t index_offset, pos_offset, attr_offset;   // of the mesh in SceneView::indices, `pos`, SceneView::attributes
    uint32_t cap_verts, cap_indices;                  // capacities of the vertex and index pools
    const float4* pos;                // object-space positions of every mesh (already the new ones)
    float4* block;                    // [nverts] decoded normals of this call
    float4* pool_normals;             // PoolState::d_normals, or null
    const uint32_t* reject;           // as DeformArgs::reject
    // lib/libfrt_exp.so only (FRT_NORMALS_TRI_PASS=1), the design that was measured and not kept: a first launch, one thread per triangle, writes the
    // triangle's normal here ([nidx / 3], call-owned scratch) and the vertex threads gather 16 bytes per corner instead of recomputing. Null in the product.
    float4* tri_scratch = nullptr;
};
hipError_t launch_vertex_normals(const SceneView& sc, const NormalArgs& a, hipStream_t stream);

// Device input: the caller's positions (and attributes) are device memory. `reject`: [0] the flag of this call, zeroed on the stream in front of the
// validation launch; [1] the calls rejected so far. The validation launch (one thread per float4 of the input) raises the flag for a non-finite float;
// the copy-in launch (one thread per vertex) returns at once when it is raised — its first thread then counts the rejection — and otherwise copies the
// vertex into the pools and, when `block` is given (attributes without FRT_DEFORM_RECOMPUTE_NORMALS), decodes its normal as mesh_append_kernel does.
struct DeformInput {
    const float4* pos; const float4* attrs;           // the caller's: [nverts] and [2 nverts] (or null)
    uint32_t nverts, pos_offset, attr_offset, cap_verts;
    float4* out_pos; float4* out_attrs;               // the replica's pools
    float4* block; float4* pool_normals;              // decoded normals, as NormalArgs (both may be null)
    uint32_t* reject;
};
// Zeroes the flag, validates, copies in.
hipError_t launch_deform_input(const DeformInput& a, hipStream_t stream);

// Words 0..23 of a shading record (frt_shade.hpp: fetch_hit_geometry), shared with frt_instance_edit.hip: a gather, no arithmetic.
//   q0 (n0.xyz, uv0.x) q1 (n1.xyz, uv0.y) q2 (n2.xyz, uv1.x) q3 (t0.xyz, uv1.y) q4 (t1.xyz, uv2.x) q5 (t2.xyz, uv2.y); q6 = (tangent sign of corner 0, mat_id, 0, 0)
// `n`: the decoded normals of the three corners; `nu`, `tg`: the two float4 of their attributes, (normal.xy, uv.xy) and (tangent.xyzw).
__device__ inline void store_shade_corners(float4* rec, const float4 n[3], const float4 nu[3], const float4 tg[3]) {
    rec[0] = make_float4(n[0].x, n[0].y, n[0].z, nu[0].z);
    rec[1] = make_float4(n[1].x, n[1].y, n[1].z, nu[0].w);
    rec[2] = make_float4(n[2].x, n[2].y, n[2].z, nu[1].z);
    rec[3] = make_float4(tg[0].x, tg[0].y, tg[0].z, nu[1].w);
    rec[4] = make_float4(tg[1].x, tg[1].y, tg[1].z, nu[2].z);
    rec[5] = make_float4(tg[2].x, tg[2].y, tg[2].z, nu[2].w);
}

// The triangle (and shading record) rewrite on `stream`. Launches nothing when there is no work.
hipError_t launch_mesh_deform(const SceneView& sc, const DeformArgs& a, hipStream_t stream);

} // namespace frt
