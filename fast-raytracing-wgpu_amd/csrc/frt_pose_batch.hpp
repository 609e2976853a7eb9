// frt_pose_batch.hpp — device side of every call that poses meshes ("Posing several meshes"): n meshes posed under one palette and/or one
// weight vector by launches whose number does not depend on n. frt_renderer_set_mesh_poses is the call; frt_renderer_set_mesh_pose(_ex) and
// _set_mesh_morph_weights are the batch of one mesh. frt_renderer_animate_cast ("Animating a cast") runs the same launches with a palette and weights of
// its own per mesh: every segment names the ones it is posed under, and set_mesh_poses is the case where all segments name the same. The kernels are
// segmented: a thread handles one vertex (or triangle) of the concatenation of the batch's meshes and finds its mesh in the call's segment table by a
// binary search over prefix sums. The arithmetic is the host specification's own functions — morphed_position, skinned_position, skinned_position_dq,
// recomputed_vertex_normal, decode_octahedral_normal, instance_world_vertices — and every vertex and triangle is computed from its own mesh alone, so a
// batch gives, bit for bit, what the n single calls give. The host specification is SceneBuilder::set_mesh_poses (frt_scene.cpp).
#pragma once
#include "frt_deform.hpp"
#include "frt_skin.hpp"
#include "frt_morph.hpp"

namespace frt {

// One mesh of the batch, 80 B, built on the host and copied up with the call (five 16-byte loads).
struct PoseSegment {
    uint32_t vert_begin;      // the mesh's first vertex in the batch's scratch: the prefix sum of nverts over the records before this one
    uint32_t nverts;
    uint32_t pos_offset;      // of the mesh's first vertex in the object-space positions
    uint32_t attr_offset;     // ... in SceneView::attributes (and the pool of decoded normals)
    uint32_t index_offset;    // of the mesh in SceneView::indices
    uint32_t ntris;
    const uint8_t* skin;      // RefitState::MeshBinding of the skin: [bind positions 16 nverts | weights 16 nverts | joints 8 nverts], or null
    const uint8_t* morph;     // ... of the morph targets: [base positions 16 nverts | deltas, target-major, 12 nverts per target], or null
    const uint32_t* adj;      // the mesh's vertex -> corner adjacency, [offsets: nverts + 1 | corners: 3 ntris], or null (normals kept)
    const float4* palette;    // [4 njoints] columns this mesh is skinned under (`skin` given), else null
    const float* weights;     // [ntargets] this mesh is morphed under (`morph` given), else null
    uint32_t njoints, ntargets;
    uint32_t skin_mode;       // how `skin` is posed: 0 the linear blend, FRT_SKIN_DUAL_QUATERNION (the mode the mesh was bound with)
    uint32_t pad;             // (16-byte loads: the record is a multiple of 16 bytes)
};
static_assert(sizeof(PoseSegment) == 80 && sizeof(PoseSegment) % 16 == 0, "PoseSegment layout");

// Everything the launches of one call share. All launches run on the renderer's main stream in the order below; what one writes the next reads behind
// the kernel boundary, and nothing is passed between the blocks of a launch. A wave may hold vertices of several meshes: every thread looks its own
// segment up. `total`: the summed vertex counts; no thread stores at or past `scratch_len` in a scratch or at or past a pool's capacity.
struct PoseBatchArgs {
    const PoseSegment* seg; uint32_t nseg, total;
    uint32_t skins, morphs;   // segments with a skin / with morph targets: a skin launch / the morph launch runs
    uint32_t skins_dq;        // of `skins`, those bound with FRT_SKIN_DUAL_QUATERNION: the dual-quaternion launch runs; fewer than `skins`: the linear one
    // Device memory the host has not seen, tested by the first skin launch of the call and the morph launch: ONE range each per call, which holds every palette (weight
    // vector) a segment names. check_palette [check_cols] float4, check_weights [check_nweights]; null: the values came from the host, which checked them.
    const float4* check_palette; uint32_t check_cols;
    const float* check_weights; uint32_t check_nweights;
    float4* morphed;          // [scratch_len] scratch of the morph launch for the segments a skin launch then reads, else null
    float4* skinned;          // [scratch_len] the posed positions of this call
    uint32_t scratch_len;
    float4* out_pos;          // the object-space positions of every mesh
    float4* block;            // [total] decoded normals of this call (recompute), or null: normals and shading records stay
    float4* pool_normals;     // PoolState::d_normals, or null
    uint32_t cap_verts, cap_indices;
    uint32_t* reject;         // DeformInput::reject
    // the triangle rewrite: one DeformInstance per instance of a mesh of the batch, work_begin running over all of them, and per record its segment
    const DeformInstance* rec; const uint32_t* rec_seg; uint32_t nrec, work;
    const uint32_t* slot_of;
    // [4 per instance] the matrix table of the device-input transforms (DeviceTransformState::m), or null. Given: the triangle launch takes a record's
    // matrix from the table, by the record's instance id, and not from the record (whose copy would have come from the host's mirror, behind a wait).
    const float4* inst_m; uint32_t num_inst;
};

// Zeroes the flag, then the morph launch and/or the skin launches (`morphs`, `skins`; a segment with both is morphed into `morphed`, which its skin
// reads): the linear launch when a skinned segment is linear, the dual-quaternion launch when one is not, each over the segments of its own mode,
// the validation launch over `skinned`, the copy-in launch into `out_pos`, the normal launch (when `block` is given) and the triangle launch (when there
// is work). The scene-extent pass and the refit follow in the caller, once.
hipError_t launch_pose_batch(const SceneView& sc, const PoseBatchArgs& a, hipStream_t stream);

} // namespace frt
