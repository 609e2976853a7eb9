// frt_scene.hpp — host-side scene model: C++ mirror of the reference's SceneBuilder / geometry / scenes API
// (src/scene/builder.rs, src/geometry.rs, src/scene/scenes.rs) with the driver-built BLAS/TLAS replaced by an
// explicit host SAH-BVH over the flattened world-space triangle list.
#pragma once
#include "../../include/frt.h"
#include "frt_bvh8.hpp"
#include <vector>
#include <string>
#include <stdint.h>

namespace frt {

struct Mat4 { float m[16]; };   // column-major, m[4*c + r]

Mat4 mat4_identity();
Mat4 mat4_mul(const Mat4& a, const Mat4& b);
Mat4 mat4_translation(float x, float y, float z);
Mat4 mat4_scale(float x, float y, float z);
Mat4 mat4_rotation_x(float a);
Mat4 mat4_rotation_y(float a);
Mat4 mat4_rotation_z(float a);
Mat4 mat4_inverse(const Mat4& a);

// src/geometry.rs:12-18 (no BLAS handle: the acceleration structure is built in SceneBuilder::build)
struct Geometry {
    std::vector<float> positions;            // xyzw per vertex
    std::vector<frt_vertex_attr> attributes;
    std::vector<uint32_t> indices;
};
namespace geometry {
void encode_octahedral_normal(const float n[3], float out[2]);   // geometry.rs:56
Geometry create_plane();                                         // geometry.rs:79  create_plane_blas
Geometry create_cube();                                          // geometry.rs:120 create_cube_blas
Geometry create_sphere(uint32_t subdivisions);                   // geometry.rs:222 create_sphere_blas
Geometry create_crystal();                                       // geometry.rs:350 create_crystal_blas
}

// src/scene/material.rs builder-style helpers
struct MaterialBuilder {
    frt_material m;
    explicit MaterialBuilder(float r, float g, float b, float a);   // Material::new, :31
    MaterialBuilder& light_index(int32_t i) { m.light_index = i; return *this; }
    MaterialBuilder& metallic(float roughness) { m.metallic = 1.0f; m.roughness = roughness; return *this; }   // :54-58 (sic)
    MaterialBuilder& roughness(float r) { m.roughness = r; return *this; }
    MaterialBuilder& glass(float ior) { m.metallic = 0.0f; m.roughness = 0.0f; m.ior = ior; m.transmission = 1.0f; return *this; }
    MaterialBuilder& texture(uint32_t id) { m.tex_info_0 = (m.tex_info_0 & 0xFFFF0000u) | (id & 0xFFFFu); return *this; }
    MaterialBuilder& emissive_factor(float r, float g, float b) { m.emissive_factor[0] = r; m.emissive_factor[1] = g; m.emissive_factor[2] = b; return *this; }
    operator frt_material() const { return m; }
};

struct MeshInfo { uint32_t vertex_offset, index_offset, pad[2]; };   // src/scene/resources.rs:2-8

struct InstanceRec {     // TLAS instance (builder.rs:181-189) + derived data
    uint32_t mesh_id, mat_id, first_tri, tri_count, flip;
    float m[16];
    float w2o[9];        // world_to_object 3x3: w2o[3*c + r]
    int32_t light = -1;  // the light register_quad_light / register_sphere_light added with this instance (moves with it), or -1
    uint32_t light_kind = 0;   // 0 quad, 1 sphere
};

struct TriRec { float v0[3], e1[3], e2[3]; };

// GPU layouts -------------------------------------------------------------------------------------------
// Pair node, 64 B: the boxes of both children of one BVH2 inner node + two child references.
//   one float4 per axis: qa = (c0.min.a, c1.min.a, c0.max.a, c1.max.a) for a = x, y, z (pairs for v_pk_fma_f32, frt_trace.hpp: slab2);
//   q3 = (ref0, ref1, 0, 0) as bits
// ref: bit 31 clear -> pair-node index; bit 31 set -> leaf: bits 0..23 first triangle slot, bits 24..30 triangle count.
// An absent child has ref = 0xFFFFFFFF and an inverted box.
struct PairNode { float q[16]; };
struct QuadNode { float q[32]; };   // frt_trace.hpp: trace4 (four child boxes per node, 128 B)
// Triangle slot, 48 B, in leaf order: (v0.xyz, flattened id bits) (e1.xyz, instance index bits) (e2.xyz, 0)
struct TriSlot { float q[12]; };
// Shading record, 128 B per flattened triangle (frt_shade.hpp: fetch_hit_geometry)
struct ShadeTri { float q[32]; };
struct InstanceDev { uint32_t mesh_id, mat_id, first_tri, flip; float w2o[9]; float pad[3]; };   // 64 B

static const uint32_t kLeafFlag = 0x80000000u;
static const uint32_t kNoChild = 0xFFFFFFFFu;
static const int kMaxBvhDepth = 30;     // traversal stack (frt_trace.hpp kStackDepth = 32) must cover it

class SceneBuilder {
public:
    SceneBuilder();                                    // builder.rs:24 (+ default textures :41-91)
    uint32_t add_mesh(const Geometry& g);              // :123
    uint32_t add_material(const frt_material& m);      // :117
    void add_instance(uint32_t mesh_id, uint32_t mat_id, const Mat4& transform);   // :181 (mask ignored, as there)
    uint32_t add_light(const frt_light& l);
    void register_quad_light(uint32_t mesh_id, const Mat4& t, const float color[3], float intensity);     // :316
    void register_sphere_light(uint32_t mesh_id, const Mat4& t, const float color[3], float intensity);   // :353
    void add_quad_light(const float pos[3], const float u[3], const float v[3], const float emission[4]);   // :392
    void add_sphere_light(const float center[3], float radius, const float emission[4]);                   // :418
    uint32_t add_color_texture(const uint8_t* rgba8);  // :93
    uint32_t add_data_texture(const uint8_t* rgba8);   // :105
    void build();                                      // :431 — flatten + SAH BVH (host only)
    // New transforms for instances of a built scene: the same tree and leaf order, the moved instances' triangles and
    // registered lights recomputed as build() computes them, every box refit. The specification the device refit matches bit for bit.
    // Returns an FRT_ERR_* code with `error` set, or FRT_OK.
    int set_instance_transforms(uint32_t n, const uint32_t* ids, const float* mats);
    // New vertices for one mesh of a built scene ("Deforming meshes"): the same topology, tree and leaf order; the triangles of
    // every instance of the mesh recomputed under its current matrix and, when `attrs` is given, their shading records as build() computes them;
    // every box refit. attrs == nullptr keeps the attributes and the shading records. The specification the device path matches bit for bit.
    // flags (include/frt.h): FRT_DEFORM_RECOMPUTE_NORMALS replaces the normal of every vertex by the normalised sum of the area-weighted normals of the
    // triangles around it, in the new positions (frt_vertex_normal.hpp: recomputed_vertex_normal), and recomputes the shading records as if `attrs` had held it.
    int set_mesh_vertices(uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags = 0);
    // Linear-blend skinning ("Skinning"). set_mesh_skin binds four joint indices and four weights per vertex to a mesh of a built scene; the
    // mesh's object-space positions as they are at the call are copied and become the bind pose. No vertex and no triangle changes. joints4 == nullptr
    // removes the skin. Refused, with nothing changed (check_mesh_skin): a vertex count that is not the mesh's, njoints == 0 or above 65,536 (a joint
    // index is 16 bits), a joint index >= njoints, a weight that is negative or not finite.
    // `skin_flags`: the mode the mesh is posed in from then on, 0 (the linear blend) or FRT_SKIN_DUAL_QUATERNION ("Dual-quaternion
    // skinning": frt_skin.hpp's skinned_position_dq); any other bit is refused. Binding again replaces the mode with the skin.
    int set_mesh_skin(uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t skin_flags = 0);
    // Every vertex of the bind pose through frt_skin.hpp's skinned_position under the palette `joint_mats` (njoints column-major 4x4), then
    // set_mesh_vertices(mesh_id, skinned, nullptr, nverts, flags). Refused, with nothing changed: a mesh without a skin, njoints that is not the bound
    // count, a matrix entry or a skinned coordinate that is not finite, FRT_DEFORM_DEVICE, an unknown flag bit. A set_mesh_vertices on a skinned mesh
    // leaves the bind pose as it is; remove_meshes drops the skin of a mesh that leaves and the survivors' skins follow their ids.
    int set_mesh_pose(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags = 0);
    // Morph targets ("Morph targets"). set_mesh_morph_targets binds ntargets sets of per-vertex position deltas, [ntargets][nverts][3], to
    // a mesh of a built scene; the mesh's object-space positions as they are at the call are copied and become the base. No vertex and no triangle
    // changes. deltas3 == nullptr removes the binding. Refused, with nothing changed (check_mesh_morph_targets): a vertex count that is not the mesh's,
    // ntargets == 0 or above FRT_MAX_MORPH_TARGETS, a delta that is not finite.
    int set_mesh_morph_targets(uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets);
    // Every vertex of the base through frt_morph.hpp's morphed_position under `weights`, then set_mesh_vertices(mesh_id, morphed, nullptr, nverts, flags).
    // Refused, with nothing changed: a mesh with no targets, ntargets that is not the bound count, a weight or a morphed coordinate that is not finite,
    // FRT_DEFORM_DEVICE, an unknown flag bit. A set_mesh_vertices on the mesh leaves the base as it is; remove_meshes drops the targets of a mesh that
    // leaves and the survivors' targets follow their ids.
    int set_mesh_morph_weights(uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags = 0);
    // Morph, then skin: set_mesh_pose with the morphed position (from the morph base) in the place of the skin's bind pose, which is not read.
    // morph_weights == nullptr with ntargets == 0: set_mesh_pose. Refuses what either part refuses.
    int set_mesh_pose_ex(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags = 0);
    // Several meshes under one palette and/or one weight vector ("Posing several meshes"): palette only skins, weights only morph, both morph
    // then skin, for every mesh of the call alike. All or nothing: every mesh is checked as its single call checks it and every posed vertex is computed
    // before the first mesh changes; then the meshes are applied in the order given through set_mesh_vertices. Refused besides, with nothing changed:
    // n == 0 or above FRT_MAX_POSE_MESHES, a mesh id twice, neither palette nor weights.
    int set_mesh_poses(uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags = 0);
    // What a built scene LOOKS like: no triangle, slot or box moves. Each is the specification its device form matches bit for bit,
    // validates everything before it applies anything, and leaves the scene equal to one built from scratch with the edited values.
    // Material ids[k] becomes mats[k], under the checks build() makes on a material (check_material).
    int set_materials(uint32_t n, const uint32_t* ids, const frt_material* mats);
    // Instance instance_ids[k] uses material material_ids[k]: its record, its device record and word 25 of its triangles' shading records. An instance
    // that register_*_light created is refused: its material carries the light link that set_light_emission relies on.
    int set_instance_materials(uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids);
    // lights[light].emission = (colour, intensity); a light registered with an instance also gets that instance's material re-emitted as
    // register_*_light makes it (emissive_factor = colour * intensity).
    int set_light_emission(uint32_t light, const float color[3], float intensity);
    // Overwrite one existing texture layer (kind 0 colour, 1 data).
    int set_texture(int kind, uint32_t layer, const uint8_t* rgba8);
    // How many instances a built scene holds. Each validates everything before it applies anything and leaves the scene equal, selector
    // for selector, to one built from scratch with the resulting instance list: the list is edited and build() runs again. The specification the
    // device forms match. add_instances appends in argument order and returns the id of the first new instance (the instance count when n == 0).
    int add_instances(uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats);
    // The instances `ids` leave (an id given twice leaves once); ids and flattened triangle ids above them shift down, as in a from-scratch build. An
    // instance that register_*_light created is refused, and so is removing every instance.
    int remove_instances(uint32_t n, const uint32_t* ids);
    // What a built scene no longer holds. Each validates everything before it applies anything, edits the builder's lists and runs build()
    // again: the scene then equals, selector for selector, one built from scratch with the surviving builder calls. Ids stay dense: everything above a
    // removed id shifts down, an id given twice leaves once. The specifications the device forms match.
    // Materials no instance uses (a material register_*_light made leaves with its light); the material word of every instance follows.
    int remove_materials(uint32_t n, const uint32_t* ids);
    // Meshes no instance uses: the vertex, index and mesh-info lists close up, the mesh word of every instance follows.
    int remove_meshes(uint32_t n, const uint32_t* ids);
    // Lights: a light of add_light loses its record; a light of register_*_light leaves as the composite that call made (record, instance, emissive
    // material). light_index of every material and the light link of every instance follow.
    int remove_lights(uint32_t n, const uint32_t* ids);
    // One texture layer (kind 0 colour, 1 data) no material slot of that kind names; the slots above it follow.
    int remove_texture(int kind, uint32_t layer);

    // SceneResources-equivalent host data (src/scene/resources.rs:10-22)
    std::vector<frt_material> materials;
    std::vector<frt_vertex_attr> attributes;
    std::vector<uint32_t> indices;
    std::vector<MeshInfo> mesh_infos;
    std::vector<frt_light> lights;
    std::vector<std::vector<uint8_t>> color_textures, data_textures;
    std::vector<std::vector<float>> mesh_positions;
    std::vector<uint32_t> mesh_index_counts;
    std::vector<InstanceRec> instances;
    // Per mesh its skin (set_mesh_skin); njoints == 0: none. Shorter than the mesh list while the last meshes have none.
    struct MeshSkin { uint32_t njoints = 0, mode = 0; std::vector<uint16_t> joints; std::vector<float> weights, bind; };
    std::vector<MeshSkin> mesh_skins;
    // Per mesh its morph targets (set_mesh_morph_targets); ntargets == 0: none. Shorter than the mesh list while the last meshes have none.
    struct MeshMorph { uint32_t ntargets = 0; std::vector<float> deltas, base; };      // deltas [ntargets][nverts][3], base [nverts][4]
    std::vector<MeshMorph> mesh_morphs;
private:
    int check_mesh_call(const char* call, const char* renderer_call, uint32_t mesh_id, uint32_t flags);      // the preamble of the mesh-edit calls (frt_scene.cpp)
    // What set_mesh_pose_ex would apply to the mesh, or what refuses it (`check_inputs`: the palette's and the weights' entries are read for finiteness).
    std::string pose_mesh(uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, bool check_inputs, std::vector<float>& posed) const;
public:
    // built
    bool built = false;
    std::vector<TriRec> tris;
    std::vector<uint32_t> tri_instance;
    std::vector<frt_bvh2_node> bvh2;
    std::vector<uint32_t> bvh2_tri_index;
    uint32_t bvh_depth = 0, bvh_leaves = 0, bvh_max_leaf = 0;
    std::vector<PairNode> pair_nodes;
    std::vector<QuadNode> quad_nodes;       // the same tree with every other level folded away (build_quad_nodes)
    uint32_t quad_stack_need = 0;           // deepest traversal stack a ray can need in the quad tree
    uint32_t quad_fold = 0;                 // how the quad tree was folded (frt_bvh.cpp: build_quad_nodes): 2 surface-area programme, 1 programme + greedy where the stack bound asks, 0 greedy
    std::vector<uint32_t> qnode_a, qnode_b;     // quantized pair nodes, 4 words per node each (frt_trace.hpp: QBvh)
    float qmin[3] = {0, 0, 0}, qstep[3] = {1, 1, 1};
    std::vector<TriSlot> tri_slots;
    std::vector<uint32_t> tri_slot_of;      // flattened triangle id -> its slot in tri_slots (the inverse of bvh2_tri_index)
    // The same tree as 8-wide nodes with grid boxes (frt_bvh8.hpp; frt_trace.hpp: trace8), built on first use (ensure_wide8): the product's kernels walk
    // the quad tree; the 8-wide walk is an experiment (lib/libfrt_exp.so) and its tree is otherwise read by tests and tools/bvh_quality.cpp only.
    mutable Wide8 wide8;                    // wide8.ok = false: not walkable that way (more than 65,536 nodes)
    mutable std::vector<TriSlot> tri_slots8;   // the triangle slots in the wide tree's order (a node's leaf triangles contiguous)
    mutable bool wide8_built = false;
    void ensure_wide8() const;
    std::vector<ShadeTri> shade_tris;
    std::vector<InstanceDev> instances_dev;
    float srgb_lut[256];
    std::string error;

private:
    void flatten();
    void refit();
    void build_bvh2();
    void build_gpu_layout();
    void write_shade_tri(uint32_t id);      // shade_tris[id] from the attributes of its three corners and its instance's material
};

// Derived data of one instance transform, as flatten() computes it: world_to_object by cofactors in double, rounded once to f32, and the
// flip flag. False (outputs untouched) when the matrix has a non-finite entry or a singular 3x3.
bool instance_inverse(const float m[16], float w2o[9], uint32_t& flip);
// One world-space triangle of an instance (the contract of DESIGN.md §3): p = ((c0*x + c1*y) + c2*z) + c3 in f32, e1 = v1 - v0, e2 = v2 - v0.
void world_triangle(const float m[16], const float* pos4, const uint32_t idx[3], TriRec& out);
// The light record register_quad_light / register_sphere_light make for transform t (emission = (colour, intensity)).
frt_light quad_light_record(const Mat4& t, const float emission[4]);
frt_light sphere_light_record(const Mat4& t, const float emission[4]);
// Argument checks shared by the scene and the renderer form of set_instance_transforms: "" when (n, ids, mats) may be applied.
std::string check_instance_transforms(uint32_t n, const uint32_t* ids, const float* mats, size_t num_instances);
// Argument checks shared by the scene and the renderer form of set_mesh_vertices: "" when the vertices may be applied to a mesh of
// `mesh_nverts` vertices (mesh_id < num_meshes is checked by the caller, which looks that count up).
std::string check_mesh_vertices(const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t mesh_nverts);
// Argument checks shared by the scene and the renderer forms of set_mesh_skin and set_mesh_pose: "" when the call may be applied to a mesh of
// `mesh_nverts` vertices, or under a skin of `bound_joints` joints (0: the mesh has no skin). Whether the skinned coordinates are finite is for the
// caller to find out: the scene computes them, the renderer's validation launch reads them.
std::string check_mesh_skin(const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t mesh_nverts);
std::string check_mesh_pose(const float* joint_mats, uint32_t njoints, uint32_t bound_joints, bool host_memory = true);      // (device memory: the matrices are not read)
// The same for set_mesh_morph_targets and for the weights of set_mesh_morph_weights and set_mesh_pose_ex: "" when the call may be applied to a mesh of
// `mesh_nverts` vertices, or under `bound_targets` bound targets (0: the mesh has none). Whether the morphed coordinates are finite is for the caller
// to find out, as with a pose.
std::string check_mesh_morph_targets(const float* deltas3, uint32_t nverts, uint32_t ntargets, uint32_t mesh_nverts);
std::string check_mesh_morph_weights(const float* weights, uint32_t ntargets, uint32_t bound_targets, bool host_memory = true);      // (device memory: the weights are not read)
// What the scene and the renderer form of set_mesh_poses check about the batch itself: "" when mesh_ids [n] names 1 to FRT_MAX_POSE_MESHES different
// meshes of a scene with num_meshes meshes and the call gives a palette, morph weights or both.
std::string check_pose_batch(uint32_t n, const uint32_t* mesh_ids, size_t num_meshes, bool palette, bool weights);
// The vertex -> corner adjacency of one mesh in CSR form: corners[offsets[v] .. offsets[v + 1]) are the corners 3 * triangle + k whose index is v,
// ascending. offsets has nverts + 1 entries, corners nidx (an index out of range, which the checks let into no mesh, names no vertex).
void build_vertex_corners(const uint32_t* idx, uint32_t nidx, uint32_t nverts, std::vector<uint32_t>& offsets, std::vector<uint32_t>& corners);
// What build() and set_materials check on a material, whose texture layers and light index reach the kernels unchecked: "" when all five layers exist
// (or are 0xFFFF) and light_index < num_lights (or is negative).
std::string check_material(const frt_material& m, size_t color_layers, size_t data_layers, size_t num_lights);
// Argument checks shared by the scene and the renderer forms of the material edits: "" when the call may be applied.
std::string check_set_materials(uint32_t n, const uint32_t* ids, const frt_material* mats, size_t num_materials, size_t color_layers, size_t data_layers, size_t num_lights);
std::string check_set_instance_materials(uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids, const std::vector<InstanceRec>& instances, size_t num_materials);
std::string check_set_texture(int kind, uint32_t layer, const uint8_t* rgba8, size_t color_layers, size_t data_layers);
// Argument checks shared by the scene and the renderer forms of add_instances / remove_instances: FRT_OK, or the code with `why` set.
// `mesh_tris`: triangles per mesh; `num_tris`: flattened triangles now. remove: `removed` receives the distinct ids, ascending.
static const uint64_t kMaxSceneTris = 0xFFFFFFFEull;
int check_add_instances(uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats, const std::vector<uint32_t>& mesh_tris, size_t num_materials,
                        uint64_t num_tris, std::string& why);
int check_remove_instances(uint32_t n, const uint32_t* ids, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why);
// emissive_factor of the material register_*_light makes for (colour, intensity): colour[k] * intensity in f32.
void light_emissive_factor(const float color[3], float intensity, float out[3]);
// The material register_*_light makes for its instance: white, emissive, linked to light `light_index`.
frt_material light_emissive_material(size_t light_index, const float color[3], float intensity);
// Argument checks of the calls that add meshes, materials, texture layers and lights to a renderer's replica: FRT_OK, or the code with
// `why` set. The counts are the replica's as they are; nothing here knows a device, so a stand-alone host program can call them.
static const uint64_t kMaxPoolElems = 0xFFFFFFFFull;      // vertices and indices are addressed with 32 bits
static const size_t kMaxMaterials = 0xFFFFu;            // (frt_scene_add_material)
static const size_t kMaxTextureLayers = 0xFFFEu;        // a texture array of a replica: a 65,535th layer is refused (0xFFFF means "none" in tex_info_*)
int check_add_meshes(uint32_t n, const frt_mesh_data* meshes, uint64_t num_verts, uint64_t num_indices, std::string& why);
int check_add_materials(uint32_t n, const frt_material* mats, size_t num_materials, size_t color_layers, size_t data_layers, size_t num_lights, std::string& why);
int check_add_texture(int kind, const uint8_t* rgba8, size_t color_layers, size_t data_layers, std::string& why);
int check_add_lights(uint32_t n, const frt_light* lights, std::string& why);
// One appended mesh of a call, 32 B, as mesh_append_kernel reads it (frt_mesh_edit.hpp): where its vertices and indices go in the replica's pools, how
// many there are, and where they begin among the call's staged vertices and indices (prefix sums over the meshes before it).
struct MeshAppend { uint32_t vert_base, index_base, nverts, nidx, vert_begin, index_begin, pad[2]; };
static_assert(sizeof(MeshAppend) == 32, "MeshAppend layout");
// The records of a call that passed check_add_meshes, for pools that hold num_verts vertices and num_indices indices; returns the call's totals.
void pack_mesh_appends(uint32_t n, const frt_mesh_data* meshes, uint32_t num_verts, uint32_t num_indices, std::vector<MeshAppend>& rec, uint32_t& new_verts, uint32_t& new_indices);
// The capacity a pool of `have` elements gets when `need` no longer fit: at least twice as many, never beyond `limit`.
uint32_t grown_capacity(uint64_t have, uint64_t need, uint64_t limit);
// ... and a texture array, whose layers are 4 MiB each: max(4, have / 2) layers more, or what is needed.
uint32_t grown_layer_capacity(uint64_t have, uint64_t need);
// The instance a light was registered with, or -1 (a light of add_light / add_*_light).
int light_instance(const std::vector<InstanceRec>& instances, uint32_t light);
static const size_t kTextureLayerBytes = 1024u * 1024u * 4u;   // src/scene/mod.rs:12-13
// Removing materials, meshes, lights and texture layers: the argument checks and the renumbering shared by the scene forms, the renderer
// forms and a stand-alone host program. Nothing here knows a device. The checks return FRT_OK or the code with `why` set; `removed` receives the distinct
// ids, ascending.
static const uint32_t kGone = 0xFFFFFFFFu;             // in an old -> new table: the id left
static const uint32_t kBuilderLayers = 3u;             // the layers of each kind SceneBuilder() makes itself: never removed
static const float kGoneMaterialWord = 65535.0f;       // gpos.w of a pixel whose material left: no valid id (kMaxMaterials ids: 0 .. 65,534)
// old -> new ids of `count` dense ids after the ascending, distinct ids `removed` left.
std::vector<uint32_t> removal_map(size_t count, const std::vector<uint32_t>& removed);
// `list` without the elements `removed` names (ascending, distinct), the survivors in their order.
template <class T>
void remove_elements(std::vector<T>& list, const std::vector<uint32_t>& removed) {
    size_t g = 0, w = 0;
    for (size_t i = 0; i < list.size(); ++i) {
        if (g < removed.size() && removed[g] == i) { ++g; continue; }
        if (w != i) list[w] = std::move(list[i]);
        ++w;
    }
    list.resize(w);
}
int check_remove_materials(uint32_t n, const uint32_t* ids, size_t num_materials, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why);
int check_remove_meshes(uint32_t n, const uint32_t* ids, size_t num_meshes, const std::vector<InstanceRec>& instances, std::vector<uint32_t>& removed, std::string& why);
// What a call of remove_lights takes out: the lights, the instances registered with them and those instances' materials (each ascending, distinct).
struct LightRemoval { std::vector<uint32_t> lights, instances, materials; };
// `materials`: the scene's or the replica's material records as they are (their light_index is what the check reads).
int check_remove_lights(uint32_t n, const uint32_t* ids, size_t num_lights, const frt_material* materials, size_t num_materials, const std::vector<InstanceRec>& instances,
                        LightRemoval& out, std::string& why);
int check_remove_texture(int kind, uint32_t layer, size_t color_layers, size_t data_layers, const frt_material* materials, size_t num_materials, std::string& why);
// One material record under new light indices (`light_map`: old -> new, or empty) and without layer `color_layer` / `data_layer` (kGone: none left):
// light_index >= 0 and the five 16-bit slots follow, 0xFFFF and negative indices stay. What remap_material_words_kernel does word by word.
void remap_material(frt_material& m, const std::vector<uint32_t>& light_map, uint32_t color_layer, uint32_t data_layer);
// One removed mesh in one of the three pools it occupies (meshes, vertices, indices), 8 B; a table is sorted by mesh id. `new_begin`: elements that survive
// in front of the range; `through`: elements removed up to and including it. The element at new index g was at g + through of the last span with
// new_begin <= g (frt_scene_remove.hpp: removed_in_front).
struct RemovedSpan { uint32_t new_begin, through; };
// The three tables of a call that passed check_remove_meshes, one span per removed mesh each, for pools laid out by (vert_offset, vert_count,
// index_offset, index_count) per mesh.
void pack_mesh_removal(const std::vector<uint32_t>& removed, const std::vector<uint32_t>& vert_offset, const std::vector<uint32_t>& vert_count,
                       const std::vector<uint32_t>& index_offset, const std::vector<uint32_t>& index_count,
                       std::vector<RemovedSpan>& meshes, std::vector<RemovedSpan>& verts, std::vector<RemovedSpan>& indices);
// The decoded normal a shading record holds for a vertex with these attributes (frt_shade.hpp: decode_octahedral_normal, compiled for the host).
void decoded_vertex_normal(const frt_vertex_attr& a, float out[3]);

namespace scenes {
void create_cornell_box(SceneBuilder& b);    // scenes.rs:9-130
void create_restir_scene(SceneBuilder& b);   // scenes.rs:133-223
}

// src/camera.rs:207-256 at the initial pose
void camera_default(float aspect, uint32_t frame_count, uint32_t num_lights, frt_camera_uniform* out);
void camera_build_uniform(const float position[3], float yaw, float pitch, const float* prev_view_proj, float aspect, uint32_t frame_count,
                          uint32_t num_lights, float jitter_x, float jitter_y, frt_camera_uniform* out, float* unjittered_out);
void camera_halton_jitter(uint32_t index, uint32_t width, uint32_t height, float scale, float out[2]);

} // namespace frt

struct frt_scene { frt::SceneBuilder b; };
