/* frt.h — C ABI of the MI355X-native path tracer (drop-in boundary for the hot path of
 * kokutoupan/fast-raytracing-wgpu: G-buffer -> ReSTIR-PT temporal -> ReSTIR-PT spatial + shade -> post/accumulate).
 *
 * The reference has no FFI; the seam is the Rust API between `State` and `SceneBuilder` / `Renderer`
 * (src/state.rs:57-80, :192-204). Every entry point below names the reference interface it replaces.
 * All structs are byte-identical to the reference's #[repr(C)] types. Plain pointers and sizes only.
 *
 * Conventions: functions returning int return 0 (FRT_OK) or a negative frt_status; the message for the last
 * failure on the calling thread is frt_last_error(). Handles are not thread-safe (like the reference, which
 * drives everything from the winit main thread). Inputs are copied; outputs go to caller-owned buffers.
 * There is NO CPU rendering path: every render entry point fails with FRT_ERR_NO_DEVICE without a HIP device.
 */
#ifndef FRT_H
#define FRT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum frt_status {
    FRT_OK = 0,
    FRT_ERR_INVALID_ARG = -1,
    FRT_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime error: the product never falls back to the CPU */
    FRT_ERR_HIP = -3,
    FRT_ERR_STATE = -4,        /* call order (e.g. render before build) */
    FRT_ERR_LIMIT = -5         /* scene exceeds a compiled limit (BVH depth vs traversal stack, u16 ids) */
} frt_status;

/* ---- data types ------------------------------------------------------------------------- */

/* src/geometry.rs:4-10 — VertexAttributes, 32 B */
typedef struct frt_vertex_attr { float normal[2]; float uv[2]; float tangent[4]; } frt_vertex_attr;

/* src/scene/material.rs:2-28 — Material, 64 B. Texture ids are u16 pairs, 0xFFFF = none. */
typedef struct frt_material {
    float base_color[4];
    float emissive_factor[3];
    float roughness;
    float metallic, transmission, ior;
    int32_t light_index;
    uint32_t tex_info_0;   /* [base colour tex (low), normal tex (high)] */
    uint32_t tex_info_1;   /* [occlusion tex (low), emissive tex (high)] */
    uint32_t tex_info_2;   /* [metallic-roughness tex (low), pad] */
    uint32_t pad_final;
} frt_material;

/* src/scene/light.rs:1-16 — LightUniform, 64 B. type_: 0 quad, 1 sphere (v[0] = radius). */
typedef struct frt_light {
    float position[3]; uint32_t type_;
    float u[3]; float area;
    float v[3]; uint32_t pad;
    float emission[4];
} frt_light;

/* src/camera.rs:4-15 — CameraUniform, 288 B, matrices column-major. */
typedef struct frt_camera_uniform {
    float view_proj[16];
    float view_inverse[16];
    float proj_inverse[16];
    float view_pos[4];
    float prev_view_proj[16];
    uint32_t frame_count, num_lights, padding[2];
} frt_camera_uniform;

/* src/passes/restir.rs:5-14 — Reservoir, 32 B */
typedef struct frt_reservoir { uint32_t y; float w_sum; uint32_t M; float W; float s_path[3]; float p_hat; } frt_reservoir;

/* Canonical BVH2 node, 32 B (replaces the opaque driver BLAS/TLAS of src/scene/builder.rs:143-179, :454-468).
 * count > 0: leaf over tri_index[left_first .. left_first + count); count == 0: children left_first, left_first + 1. */
typedef struct frt_bvh2_node { float bmin[3]; uint32_t left_first; float bmax[3]; uint32_t count; } frt_bvh2_node;

typedef struct frt_scene frt_scene;
typedef struct frt_renderer frt_renderer;

/* ---- errors --------------------------------------------------------------------------------------------- */
const char* frt_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unavailable). Does not initialise a device context. */
int frt_device_count(void);

/* ---- geometry generators: src/geometry.rs:79-434 (create_*_blas without the wgpu BLAS handle) --------------
 * which: 0 plane (:79), 1 cube (:120), 2 icosphere(subdiv) (:222), 3 crystal (:350).
 * Call with null buffers to get counts; then with buffers of nverts*16, nverts*32, nidx*4 bytes. */
int frt_geometry_create(int which, uint32_t subdiv, uint32_t* nverts, uint32_t* nidx,
                        float* pos4, frt_vertex_attr* attrs, uint32_t* idx);
/* src/geometry.rs:56-76 */
void frt_encode_octahedral_normal(const float n[3], float out[2]);
/* src/scene/material.rs:31-47 — Material::new defaults */
void frt_material_default(const float base_color[4], frt_material* out);

/* ---- scene: src/scene/builder.rs SceneBuilder --------------------------------------------------------------- */
frt_scene* frt_scene_create(void);                                   /* SceneBuilder::new, :24 (default textures :41-91) */
void frt_scene_destroy(frt_scene* s);
int frt_scene_add_mesh(frt_scene* s, const float* pos4, uint32_t nverts, const frt_vertex_attr* attrs,
                       const uint32_t* idx, uint32_t nidx);          /* add_mesh, :123 -> mesh id */
int frt_scene_add_material(frt_scene* s, const frt_material* m);     /* add_material, :117 -> material id */
int frt_scene_add_instance(frt_scene* s, uint32_t mesh_id, uint32_t mat_id, const float m_colmajor[16]);   /* add_instance, :181 (mask ignored there too) */
int frt_scene_add_light(frt_scene* s, const frt_light* l);           /* lights.push, :406 / :420 -> light index */
int frt_scene_register_quad_light(frt_scene* s, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity);   /* :316 */
int frt_scene_register_sphere_light(frt_scene* s, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity); /* :353 */
int frt_scene_add_texture(frt_scene* s, int kind /*0 colour (sRGB), 1 data*/, const uint8_t* rgba8_1024x1024);   /* :93-115 -> layer id */
/* SceneBuilder::build, :431 — flattens instances, builds the SAH BVH on the host. No device work. */
int frt_scene_build(frt_scene* s);
/* src/scene/scenes.rs:9-130 and :133-223 — whole-scene factories (built). */
frt_scene* frt_scene_create_cornell_box(void);
frt_scene* frt_scene_create_restir_scene(void);

/* ---- model import: src/scene/loader.rs:9-181 load_gltf (+ a Wavefront OBJ subset, an extension) -------------------------
 * frt_model = the (geometries, materials, images, material_indices) tuple load_gltf returns: one geometry per mesh primitive,
 * images (PNG, JPEG) decoded and Lanczos3-resized to 1024 x 1024 RGBA8 (grey / 16-bit / arithmetic-coded files become the white fallback texture of
 * loader.rs:35-44; see frt_model_warning), materials built as loader.rs:58-99 does (metallic is always 1: material.rs:54-58).
 * Material texture slots hold IMAGE indices until frt_scene_add_gltf_materials remaps them to texture-array layers. */
typedef struct frt_model frt_model;
frt_model* frt_model_load(const char* path);                 /* .gltf / .glb / .vrm, or .obj; NULL + frt_last_error on failure */
void frt_model_destroy(frt_model* m);
int frt_model_counts(const frt_model* m, uint32_t counts[4]);      /* geometries, materials, images, warnings */
int frt_model_geometry_counts(const frt_model* m, uint32_t geo, uint32_t* nverts, uint32_t* nidx, uint32_t* material_index);
int frt_model_geometry_get(const frt_model* m, uint32_t geo, float* pos4, frt_vertex_attr* attrs, uint32_t* idx);   /* any pointer may be NULL */
int frt_model_material_get(const frt_model* m, uint32_t i, frt_material* out);
int frt_model_material_set(frt_model* m, uint32_t i, const frt_material* in);   /* scenes.rs:392-410 rewrites loaded materials before adding them */
int frt_model_image_get(const frt_model* m, uint32_t i, uint8_t* rgba8_1024x1024);
const char* frt_model_warning(const frt_model* m, uint32_t i);    /* what the reference prints to stdout; NULL past the end */
/* src/scene/builder.rs:191-292, :294-300, :302-314. ids arrays are caller-owned ([materials] / [geometries]); return = count written */
int frt_scene_add_gltf_materials(frt_scene* s, const frt_model* m, uint32_t* mat_ids);
int frt_scene_add_gltf_meshes(frt_scene* s, const frt_model* m, uint32_t* mesh_ids);
int frt_scene_add_gltf_instances(frt_scene* s, const frt_model* m, const uint32_t* mesh_ids, uint32_t n_mesh, const uint32_t* mat_ids, uint32_t n_mat,
                                 const float transform_colmajor[16]);
/* src/scene/scenes.rs:246-322 create_gltf_scene (floor plane, 15-intensity quad light, the model; built). Differs from the
 * reference in one error case: there a model that fails to load is logged and an EMPTY scene is built; here the call returns
 * NULL with the loader's message in frt_last_error (scenes without triangles cannot be built). */
frt_scene* frt_scene_create_gltf_scene(const char* path, const float model_transform_colmajor[16], const float light_transform_colmajor[16]);

/* Introspection (tests): counts[8] = tris, instances, materials, lights, meshes, attributes, indices, bvh2 nodes */
int frt_scene_counts(const frt_scene* s, uint32_t counts[8]);
/* which: 0 tris (9 f32: v0,e1,e2), 1 tri_instance (u32), 2 materials, 3 lights, 4 attributes, 5 indices, 6 mesh infos (16 B),
 * 7 instances (120 B: mesh,mat,first_tri,tri_count,flip u32; m[16]; w2o[9] f32), 8 bvh2 nodes (32 B), 9 bvh2 tri_index (u32);
 * the device forms of the tree (frt_scene_tree_stats gives the counts): 10 quad nodes (128 B), 11 8-wide compressed nodes (128 B, csrc/frt_bvh8.hpp),
 * 12 triangle slots in the 8-wide tree's order (48 B: v0, id; e1, instance; e2, 0), 13 triangle slots in BVH2 leaf order (48 B),
 * 14 the float boxes behind the 8-wide nodes' grid boxes (192 B per node: 8 x lo.xyz, hi.xyz; host data for tools/bvh_quality.cpp),
 * 15 pair nodes (64 B; frt_scene_bvh_stats gives the count), 16 device instance records (64 B: mesh, mat, first_tri, flip u32; w2o[9] f32; 3 pad),
 * 17 shading records (128 B per flattened triangle id, 8 x float4: (n0.xyz, uv0.x) (n1.xyz, uv0.y) (n2.xyz, uv1.x) (t0.xyz, uv1.y) (t1.xyz, uv2.x)
 * (t2.xyz, uv2.y) (tangent sign, material id, 0, 0) (0, 0, 0, 0); normals decoded from their octahedral form) */
int frt_scene_get(const frt_scene* s, int which, void* out);
/* Move instances of a BUILT scene: instance ids[k] gets the column-major matrix m_colmajor16[16k .. 16k+15]. The tree
 * keeps its topology and leaf order; the moved instances' triangles, their device instance records and the lights registered with them
 * (frt_scene_register_quad_light / _sphere_light; frt_scene_add_light's lights stay) are recomputed as frt_scene_build computes them, and
 * every box is refit. An id given twice ends with its last matrix. Host copy only: renderers created from the scene are not touched (their
 * replica moves with frt_renderer_set_instance_transforms). FRT_ERR_STATE: scene not built; FRT_ERR_INVALID_ARG: an id out of range, a
 * non-finite entry, a singular 3x3 (nothing is changed then). The 8-wide tree (selectors 11, 12, 14) is made again from the refit tree. */
int frt_scene_set_instance_transforms(frt_scene* s, uint32_t n, const uint32_t* ids, const float* m_colmajor16);
/* Deform one mesh of a BUILT scene ("Deforming meshes"): new object-space positions (xyzw per vertex) and, unless attrs is
 * NULL, new attributes for every vertex of mesh `mesh_id`. The topology is fixed: nverts must be the mesh's vertex count, the indices stay. The
 * triangles of every instance of the mesh are recomputed under the instance's current matrix, in their slots; with attrs their shading records
 * (selector 17) are recomputed as frt_scene_build computes them, with attrs == NULL attributes and shading records stay as they are. Every box is
 * refit; instance records and lights do not change (a registered light follows its transform, not its mesh). Afterwards the scene equals one
 * built from scratch with the new vertices. Host copy only, as frt_scene_set_instance_transforms. FRT_ERR_STATE: scene not built;
 * FRT_ERR_INVALID_ARG, nothing changed: mesh id out of range, nverts not the mesh's count, pos4 NULL, a non-finite position or attribute float. */
int frt_scene_set_mesh_vertices(frt_scene* s, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts);
/* The same call with flags ("Recomputed normals"); flags == 0 is frt_scene_set_mesh_vertices.
 * FRT_DEFORM_RECOMPUTE_NORMALS: the normal of every vertex of the mesh is computed from the new positions. For triangle j with indices (i0, i1, i2),
 * c_j = (p1 - p0) x (p2 - p0) (area-weighted, not normalised); for vertex v, s = ((0 + c_a) + c_b) + ... over every triangle corner that names v, in
 * ascending 3 j + corner (a triangle that names v twice counts twice); d = (s.x s.x + s.y s.y) + s.z s.z; n = s * (1 / sqrt(d)), all in f32 without
 * contraction; the attribute's `normal` becomes the octahedral encoding of n that the geometry generators use. A vertex no triangle names, or whose d
 * is zero or not finite, keeps its normal. With attrs, uv and tangent (and the normal of a vertex that keeps it) come from attrs; with attrs == NULL
 * they stay. Tangents are not re-orthogonalised against the new normal. The shading records of every instance of the mesh are recomputed, and the
 * scene then equals one built from scratch whose mesh carries the new positions and these attributes.
 * FRT_DEFORM_DEVICE: frt_renderer_set_mesh_vertices_ex only. FRT_ERR_INVALID_ARG, nothing changed: an unknown flag bit, FRT_DEFORM_DEVICE here. */
#define FRT_DEFORM_RECOMPUTE_NORMALS 1u
#define FRT_DEFORM_DEVICE 2u
int frt_scene_set_mesh_vertices_ex(frt_scene* s, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags);
/* Linear-blend skinning ("Skinning"). A skin is bound to a mesh of a BUILT scene once; a pose is then only the joint palette.
 * The contract, f32 without contraction and without a hand-written fma: for vertex v with bind position p = (x, y, z, w), joint indices j[0..3], weights
 * w[0..3] and the palette's column-major 4x4 matrices M (the layout of an instance transform; row 3 is ignored), for slot k and row r in 0..2
 *   q_k[r] = ((M_jk[r] * x + M_jk[4 + r] * y) + M_jk[8 + r] * z) + M_jk[12 + r]            (the expression of an instance's world-space triangle)
 *   out[r] = ((w0 * q_0[r] + w1 * q_1[r]) + w2 * q_2[r]) + w3 * q_3[r]
 * All four terms are always evaluated (a weight of 0 is not skipped), weights are used as given (not renormalised), out.w is the bind pose's w.
 * set_mesh_skin: joints4 [4 nverts] and weights4 [4 nverts] are copied, and so are the mesh's object-space positions as they are at the call: they
 * become the bind pose. No vertex and no triangle changes. joints4 == NULL removes the skin. FRT_ERR_STATE: scene not built; FRT_ERR_INVALID_ARG, nothing
 * changed: mesh id out of range, nverts not the mesh's count, njoints == 0 or above 65536, a joint index >= njoints, a weight that is negative or not finite.
 * set_mesh_pose: every vertex by the contract from the bind pose under joint_mats [16 njoints], then exactly
 * frt_scene_set_mesh_vertices_ex(s, mesh_id, skinned, NULL, nverts, flags & FRT_DEFORM_RECOMPUTE_NORMALS). FRT_ERR_INVALID_ARG, nothing changed: a mesh
 * without a skin, njoints not the bound count, a non-finite matrix entry, a non-finite skinned coordinate (a finite pose can overflow), an unknown flag
 * bit, FRT_DEFORM_DEVICE. A later frt_scene_set_mesh_vertices on a skinned mesh is allowed and leaves the bind pose untouched; frt_scene_remove_meshes
 * drops the skin of a mesh that leaves, and the survivors' skins follow their ids. */
int frt_scene_set_mesh_skin(frt_scene* s, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints);
/* Dual-quaternion skinning ("Dual-quaternion skinning"; Kavan et al.): the skin MODE of a mesh, chosen when the skin is bound.
 * set_mesh_skin_ex is set_mesh_skin with `flags`: 0 binds the linear blend above (set_mesh_skin IS this call with flags 0), FRT_SKIN_DUAL_QUATERNION
 * binds the same joints and weights to be blended as rigid transforms, which keeps the volume a linear blend loses under a twist. Any other bit:
 * FRT_ERR_INVALID_ARG, nothing changed (checked behind the built scene and the mesh id, in front of the arrays; also when joints4 is NULL).
 * Binding again replaces the mode with the skin; frt_scene_remove_meshes drops and renumbers it with the skin. No pose call takes a mode: set_mesh_pose,
 * set_mesh_pose_ex, set_mesh_poses and everything that ends in them pose each mesh in the mode it was bound with (a batch may mix them under one
 * palette; morph then skin works in either). The checks and refusals of the pose calls are those above.
 * The contract of the mode, f32 without contraction and without a hand-written fma, sqrt and 1 / sqrt exactly rounded (rsq(x) = 1 / sqrt(x) below),
 * quaternions as (x, y, z, w), dot4(a, b) = ((a.x b.x + a.y b.y) + a.z b.z) + a.w b.w,
 * cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x):
 * PER JOINT MATRIX M (column-major, row 3 not read), with n_c = (M[4c]^2 + M[4c+1]^2) + M[4c+2]^2 for c in 0..2:
 *   s = ((sqrt(n_0) + sqrt(n_1)) + sqrt(n_2)) * 0.333333343f                                    (the uniform scale)
 *   R_rc = M[4c + r] * rsq(n_c)                                                                 (the rotation; t = (R_00 + R_11) + R_22)
 *   q = the branch of the greatest of (t, R_00, R_11, R_22), the first of equals in that order:
 *     t:    (R_21 - R_12, R_02 - R_20, R_10 - R_01, 1 + t)
 *     R_00: (((1 + R_00) - R_11) - R_22, R_01 + R_10, R_02 + R_20, R_21 - R_12)
 *     R_11: (R_01 + R_10, ((1 + R_11) - R_00) - R_22, R_12 + R_21, R_02 - R_20)
 *     R_22: (R_02 + R_20, R_12 + R_21, ((1 + R_22) - R_00) - R_11, R_10 - R_01)
 *   qr = q * rsq(dot4(q, q))            (Shepperd's choice; its square root and division are this normalisation)
 *   with (tx, ty, tz) = M[12..14]:      qd = 0.5 (t, 0) qr, that is
 *     qd.x = 0.5 ((tx qr.w + ty qr.z) - tz qr.y)   qd.y = 0.5 ((ty qr.w + tz qr.x) - tx qr.z)   qd.z = 0.5 ((tz qr.w + tx qr.y) - ty qr.x)
 *     qd.w = -0.5 ((tx qr.x + ty qr.y) + tz qr.z)
 * Shear and non-uniform scale are NOT represented: the columns are normalised one by one and their lengths averaged.
 * PER VERTEX with bind position p, joints j[0..3] and weights w[0..3]: the pivot P is the first slot of greatest weight;
 *   sigma_k = dot4(qr_k, qr_P) < 0 ? -1 : 1
 *   b[c]  = ((w0 (sigma_0 dq_0[c]) + w1 (sigma_1 dq_1[c])) + w2 (sigma_2 dq_2[c])) + w3 (sigma_3 dq_3[c])        for the eight components of (qr, qd)
 *   s_b   = ((w0 s_0 + w1 s_1) + w2 s_2) + w3 s_3
 *   (r, d) = (b_r, b_d) * rsq(dot4(b_r, b_r));  u = r.xyz;  v = s_b * p.xyz
 *   out.xyz = (v + 2 cross(u, cross(u, v) + r.w v)) + 2 ((r.w d.xyz - d.w u) + cross(u, d.xyz)),   out.w = p.w
 * All four terms are always evaluated and the weights are used as given, as in the linear form. A zero column of a joint some vertex names, and a
 * blend whose real part cancels to zero, have an infinite rsq and give NaN coordinates: the pose is refused as a non-finite skinned coordinate. */
#define FRT_SKIN_DUAL_QUATERNION 1u
int frt_scene_set_mesh_skin_ex(frt_scene* s, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t flags);
int frt_scene_set_mesh_pose(frt_scene* s, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags);
/* Morph targets, or blend shapes ("Morph targets"). A set of per-vertex position deltas is bound to a mesh of a BUILT scene once; a
 * morph is then only one weight per target. The contract, f32 without contraction and without a hand-written fma: for vertex v with base position
 * b = (x, y, z, w), targets 0..T-1 with deltas d_t = (dx, dy, dz) and weights w_t, for r in 0..2
 *   m[r] = ((...((b[r] + w_0 * d_0[r]) + w_1 * d_1[r]) ...) + w_{T-1} * d_{T-1}[r])            (in target order)
 *   m[3] = b[3]
 * Every term is evaluated (a weight of 0 is not skipped); weights are used as given: they may be negative or above 1 and are not normalised. Only
 * positions are morphed; normals follow through FRT_DEFORM_RECOMPUTE_NORMALS.
 * set_mesh_morph_targets: deltas3 [ntargets][nverts][3] is copied, and so are the mesh's object-space positions as they are at the call: they become the
 * base. No vertex and no triangle changes. deltas3 == NULL removes the binding. FRT_ERR_STATE: scene not built; FRT_ERR_INVALID_ARG, nothing changed: mesh
 * id out of range, nverts not the mesh's count, ntargets == 0 or above FRT_MAX_MORPH_TARGETS, a delta that is not finite.
 * set_mesh_morph_weights: every vertex by the contract from the base under weights [ntargets], then exactly
 * frt_scene_set_mesh_vertices_ex(s, mesh_id, morphed, NULL, nverts, flags & FRT_DEFORM_RECOMPUTE_NORMALS). FRT_ERR_INVALID_ARG, nothing changed: a mesh
 * with no targets, ntargets not the bound count, a weight that is not finite, a morphed coordinate that is not finite (finite inputs can overflow), an
 * unknown flag bit, FRT_DEFORM_DEVICE. A later frt_scene_set_mesh_vertices on the mesh is allowed and leaves the base untouched;
 * frt_scene_remove_meshes drops the targets of a mesh that leaves, and the survivors' targets follow their ids.
 * set_mesh_pose_ex: morph and skin in one call, in glTF's order: skinned_position(morphed vertex, ...), that is frt_scene_set_mesh_pose with the morphed
 * position, computed from the morph base under morph_weights [ntargets], in the place of the skin's bind pose. The skin's own bind copy is not read in this
 * call, so bind the targets and the skin before the first pose: both copies are then the same rest positions. With morph_weights == NULL and
 * ntargets == 0 it is frt_scene_set_mesh_pose, bit for bit. It refuses what either part refuses. */
#define FRT_MAX_MORPH_TARGETS 4096u
int frt_scene_set_mesh_morph_targets(frt_scene* s, uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets);
int frt_scene_set_mesh_morph_weights(frt_scene* s, uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags);
int frt_scene_set_mesh_pose_ex(frt_scene* s, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* Pose several meshes in one call ("Posing several meshes"): mesh_ids [n] under ONE palette joint_mats [16 njoints] and/or ONE
 * weight vector morph_weights [ntargets], as a character's primitives share one skeleton and one set of morph weights. What is given decides the source,
 * for every mesh of the call alike: a palette only (morph_weights == NULL, ntargets == 0) skins as frt_scene_set_mesh_pose; weights only
 * (joint_mats == NULL, njoints == 0) morph as frt_scene_set_mesh_morph_weights; both morph then skin as frt_scene_set_mesh_pose_ex. Every mesh must have
 * the bindings this implies and is checked against njoints / ntargets exactly as its single call checks it.
 * The call is atomic. Everything is validated first, the posed vertices of every mesh included; then the result equals, bit for bit, the n single-mesh
 * calls in the order given. FRT_ERR_STATE: scene not built. FRT_ERR_INVALID_ARG, nothing changed: n == 0 or above FRT_MAX_POSE_MESHES, mesh_ids == NULL,
 * a mesh id out of range or given twice, neither palette nor weights, whatever the single call refuses for any mesh (a missing binding, a count that is
 * not the bound one, a non-finite entry, a posed coordinate that overflowed), an unknown flag bit, FRT_DEFORM_DEVICE. A mesh no instance uses is legal. */
#define FRT_MAX_POSE_MESHES 1024u
int frt_scene_set_mesh_poses(frt_scene* s, uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* What a BUILT scene looks like: four edits that move no triangle, slot or box. Common rules: FRT_ERR_STATE: scene not built;
 * FRT_ERR_INVALID_ARG: an id or layer out of range, a null pointer with n > 0, a failed check; everything is validated before anything is applied, so
 * a refused call changes nothing. n == 0: FRT_OK. An id given twice ends with its last value. Afterwards the scene equals one built from scratch
 * with the edited values. Host copy only: a renderer's replica is edited by the frt_renderer_* calls of the same names.
 * set_materials: material ids[k] becomes materials[k], under the checks frt_scene_build makes on a material: each of its five texture layers
 * exists or is 0xFFFF, light_index < the number of lights (or negative). */
int frt_scene_set_materials(frt_scene* s, uint32_t n, const uint32_t* ids, const frt_material* materials);
/* Instance instance_ids[k] uses material material_ids[k]: the instance record (selector 7), the device instance record (16) and word 25 of the shading
 * record (17) of every triangle of the instance. An instance made by frt_scene_register_quad_light / _sphere_light is refused: its material
 * carries the link to its light, which frt_scene_set_light_emission relies on (edit that material with frt_scene_set_materials instead). */
int frt_scene_set_instance_materials(frt_scene* s, uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids);
/* The brightness edit: light `light` emits (color, intensity). A light made by frt_scene_register_quad_light / _sphere_light also gets its
 * instance's material re-emitted as that call makes it (emissive_factor = color * intensity, in f32); a light of frt_scene_add_light only
 * gets the record change. */
int frt_scene_set_light_emission(frt_scene* s, uint32_t light, const float color[3], float intensity);
/* Replace one EXISTING texture layer; kind and pixels as frt_scene_add_texture. */
int frt_scene_set_texture(frt_scene* s, int kind /*0 colour (sRGB), 1 data*/, uint32_t layer, const uint8_t* rgba8_1024x1024);
/* How many instances a BUILT scene holds. Afterwards the scene equals, selector for selector of frt_scene_get (the trees included),
 * a scene built from scratch with the resulting instance list: the call costs a host build. Host copy only; a renderer's replica follows with
 * frt_renderer_add_instances / _remove_instances. Everything is validated before anything is applied; a refused call changes nothing.
 * add: n instances of EXISTING meshes and materials, one column-major 4x4 each, appended in argument order with the next instance ids and the next
 * flattened triangle ids. Returns the id of the first new instance (n == 0: the instance count).
 * remove: the instances `ids` leave, an id given twice once. Ids stay dense: instance ids above a removed one and flattened triangle ids above its
 * triangles shift down; a registered light keeps its link to its (renumbered) instance.
 * FRT_ERR_STATE: scene not built. FRT_ERR_INVALID_ARG: a null pointer with n > 0; an id, mesh id or material id out of range; a non-finite matrix entry or
 * a singular 3x3; removing an instance made by frt_scene_register_quad_light / _sphere_light (its material and light record carry links to it); removing
 * every instance. FRT_ERR_LIMIT: more than 0xFFFFFFFE triangles would result, or the builder refuses the new tree. */
int frt_scene_add_instances(frt_scene* s, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* m_colmajor16);
int frt_scene_remove_instances(frt_scene* s, uint32_t n, const uint32_t* ids);
/* What a BUILT scene no longer holds. Ids stay dense: everything above a removed id shifts down, an id given twice is removed once.
 * Afterwards the scene equals, selector for selector of frt_scene_get (the trees included), a scene built from scratch with the surviving builder calls:
 * the lists are edited and the scene is built again. Host copy only; a renderer's replica follows with frt_renderer_remove_*. Everything is validated before
 * anything is applied; a refused call changes nothing. n == 0: FRT_OK.
 * materials: the material word of every instance follows. Refused: a material an instance still uses; a material frt_scene_register_quad_light /
 *   _sphere_light made (remove the light instead).
 * meshes: the vertex, index and mesh-info lists close up as a from-scratch build lays them out, the mesh word of every instance follows. Refused: a mesh
 *   an instance still uses.
 * lights: a light of frt_scene_add_light loses its record; a light of frt_scene_register_quad_light / _sphere_light leaves as the composite that call
 *   made: its record, its instance and its emissive material (instance and material ids shift as after _remove_instances and _remove_materials).
 *   light_index >= 0 of every material and the light link of every instance follow. Refused: a light that the light_index of a surviving material names;
 *   a registered light whose material another instance uses; removing every instance. A scene may be left without lights.
 * texture: one layer (kind 0 colour, 1 data); the 16-bit slots of that kind above it in every material's tex_info_* follow (colour: base colour and
 *   emissive; data: normal, occlusion, metallic-roughness; 0xFFFF stays). Refused: a layer a material slot of that kind names; layers 0 - 2 of either
 *   kind, which every scene starts with.
 * FRT_ERR_STATE: scene not built. FRT_ERR_INVALID_ARG: a null pointer with n > 0, an id or layer out of range, kind not 0 or 1, the refusals above.
 * FRT_ERR_LIMIT: the builder refuses the new tree (lights). */
int frt_scene_remove_materials(frt_scene* s, uint32_t n, const uint32_t* ids);
int frt_scene_remove_meshes(frt_scene* s, uint32_t n, const uint32_t* ids);
int frt_scene_remove_lights(frt_scene* s, uint32_t n, const uint32_t* ids);
int frt_scene_remove_texture(frt_scene* s, int kind /*0 colour, 1 data*/, uint32_t layer);
/* stats[8]: quad nodes, deepest traversal stack of the quad tree, 8-wide nodes (0: the scene has no 8-wide tree: more than 65,536 nodes), deepest stack of
 * the 8-wide tree, its levels, sum of its nodes' child counts, its triangle slots, how the quad tree was folded (2 surface-area programme, 1 programme where
 * the traversal-stack bound allows and the greedy fold elsewhere, 0 greedy fold) */
int frt_scene_tree_stats(const frt_scene* s, uint32_t stats[8]);
/* bvh stats[4]: max depth, leaves, max leaf size, wide-node count */
int frt_scene_bvh_stats(const frt_scene* s, uint32_t stats[4]);

/* ---- ray queries: caller-supplied rays against the scene, what the reference gets from the Vulkan ray query ----------
 * A ray is origin + t * dir for tmin < t < tmax (both exclusive, as everywhere in this library); dir is used as given, so t is in units of its
 * length. A hit is defined without reference to any tree: the closest hit is the smallest t, ties going to the smallest
 * flattened triangle id. A ray with a non-finite origin or direction component, an all-zero direction or a NaN tmin / tmax is a miss (unoccluded),
 * decided before any walk. */
typedef struct frt_ray { float origin[3]; float tmin; float dir[3]; float tmax; } frt_ray;                      /* 32 B */
/* tri: flattened triangle id, 0xFFFFFFFF = miss (then t = -1 and every other word is 0); instance: id in add_instance order; material: the
 * instance's material id; primitive = tri - the instance's first triangle, i.e. the triangle's index within its mesh; front: 0 or 1 */
typedef struct frt_ray_hit { float t, u, v; uint32_t tri, instance, material, primitive, front; } frt_ray_hit;   /* 32 B */
#define FRT_QUERY_MAX_RAYS (1u << 26)
/* The host form, the specification of the renderer calls below: a walk of the host copy's quad tree, single-threaded. n == 0: FRT_OK, nothing
 * touched. FRT_ERR_INVALID_ARG: a null pointer with n > 0, n > FRT_QUERY_MAX_RAYS; FRT_ERR_STATE: scene not built. */
int frt_scene_trace_closest(const frt_scene* s, uint32_t n, const frt_ray* rays, frt_ray_hit* out);
int frt_scene_trace_any(const frt_scene* s, uint32_t n, const frt_ray* rays, uint8_t* occluded_out);             /* 1 = some triangle is hit */

/* ---- camera: src/camera.rs:207-256 build_uniform at the initial pose (:40-42), jitter 0 (:202-203) ------------ */
void frt_camera_default(float aspect, uint32_t frame_count, uint32_t num_lights, frt_camera_uniform* out);
/* CameraController::build_uniform, src/camera.rs:207-256, for any pose (position, yaw, pitch: the controller's state, :38-56), jitter
 * (the projection shear of :224-228; NULL = (0, 0)) and previous view-projection (NULL = the controller's initial IDENTITY, i.e. the
 * first frame, :233-238). unjittered_view_proj (16 floats, may be NULL) is the second element of the returned tuple, which the caller
 * keeps as the next frame's prev_view_proj (state.rs:172). */
int frt_camera_build_uniform(const float position[3], float yaw, float pitch, const float* prev_view_proj_colmajor, float aspect,
                             uint32_t frame_count, uint32_t num_lights, const float jitter[2], frt_camera_uniform* out, float* unjittered_view_proj);
/* CameraController::get_halton_jitter, src/camera.rs:182-205. `scale` stands for the literal 0 the reference multiplies the Halton
 * offsets by (:202-203): 0 reproduces the shipped reference (no jitter), 1 gives the sequence its comments describe. */
void frt_camera_halton_jitter(uint32_t index, uint32_t width, uint32_t height, float scale, float out[2]);

/* ---- renderer: src/renderer.rs ---------------------------------------------------------------------------- */
typedef struct frt_render_opts {
    uint32_t max_depth;       /* MAX_DEPTH, restir.wgsl:5; 0 -> 8 */
    int32_t device;           /* HIP device ordinal */
    void* stream;             /* hipStream_t to enqueue on; NULL -> a stream owned by the renderer, unless FRT_FLAG_USE_STREAM */
    uint32_t row_begin;       /* rows [row_begin, row_end) owned by this renderer (image strip); 0,0 -> whole image */
    uint32_t row_end;
    void* device_arena;       /* optional caller-owned device memory for all per-pixel buffers (frt_renderer_arena_bytes) */
    uint64_t arena_bytes;
    uint32_t flags;           /* FRT_FLAG_* */
    uint32_t motion_halo_rows;/* strips only: rows beyond the strip for which the caller keeps PREVIOUS-frame state valid (spatial reservoirs,
                                 accumulation: frt/dist.py exchanges them before the temporal stage) so that temporal reprojection and the
                                 history fetch of a MOVING camera may land there; the G-buffer halo grows to cover them. 0 = static camera.
                                 Reads that fall outside are counted in frt_stats.halo_overflow (the frame then differs from a 1-GPU frame). */
    uint32_t queue_capacity;  /* slots of each continuation queue (paths parked between two launches of a traced stage); 0 -> sized from the
                                 share of paths that reach the first cut and grown by frt_renderer_stats after an overflow. Any value is
                                 safe: a path that finds its queue full is finished in place (frt_stats.queue_overflow counts them). */
    uint32_t cut_depths[4];   /* ascending bounce depths at which the traced stages park their surviving paths in the continuation queues and resume
                                 them, dense again, in a further launch. All zero -> the library's choice (3 and 4; renderers of
                                 fewer than 0.8 M pixels: 3). cut_depths[0] = 0xFFFFFFFF -> never cut. Entries that are not ascending are skipped.
                                 Pixels do not depend on it. */
} frt_render_opts;
#define FRT_FLAG_TIMING 1u          /* record per-stage HIP events every frame (frt_stats.ms_*) */
#define FRT_FLAG_PIPELINE 8u        /* two-stream schedule: the G-buffer and the T-trace half of the temporal stage of the NEXT
                                       frame run on a second stream beside this frame's spatial continuation launches and post (the latency-bound
                                       part of the frame). The next frame's camera is speculated (this camera, frame_count + 1, prev_view_proj =
                                       view_proj: a camera that did not move) and checked against the real uniform at the next render call; a wrong
                                       guess is dropped and redone in order. Same pixels; reads, frt_renderer_sync and frt_renderer_stats see
                                       completed frames as without the flag. Callers that read the G-buffer / motion targets through
                                       frt_renderer_buffer_info on their own stream call frt_renderer_fence first. */
#define FRT_FLAG_OVERLAP_POST FRT_FLAG_PIPELINE   /* round-1 name */
#define FRT_FLAG_USE_STREAM 4u      /* opts->stream is authoritative even when NULL (= the legacy default stream, e.g. torch's current stream) */
#define FRT_FLAG_COMPACTION 2u      /* EXPERIMENTS BUILD ONLY (lib/libfrt_exp.so, `make experiments`): temporal / spatial stages through the
                                       workgroup-compacting kernels (measured slower, profiles/r1_v3_*). The product library rejects the flag. */
#define FRT_FLAG_THIRD_GSET 16u     /* with FRT_FLAG_PIPELINE: a whole-frame renderer also owns the third G-buffer / motion / candidate set (60 B per
                                       pixel outside the arena) that strip renderers own, so that the next frame's G-buffer + T-trace need not wait
                                       for this frame's T-merge. No gain for a whole frame; lets tests drive that schedule. */

/* EXPERIMENTS BUILD ONLY (lib/libfrt_exp.so, `make experiments`; the product library rejects them): round 4's two measured-and-not-kept walks. Same pixels. */
#define FRT_FLAG_WALK_WIDE 32u      /* the traced kernels walk the scene's 8-WIDE tree with 16-bit grid boxes (csrc/frt_bvh8.hpp, frt_trace.hpp: trace8; a tree of at
                                       most 28 KiB is copied into every traced workgroup's LDS) instead of the 4-wide one: Cornell Box 1.57 vs 1.54 ms per frame,
                                       larger scenes 17 - 33 % slower (profiles/r4_experiments/wide8.md) */
#define FRT_FLAG_WALK_WIDE_HBM 64u  /* the same walk with the tree read from HBM / L1 even when it would fit a workgroup's LDS */
#define FRT_FLAG_WG_TRACE 128u      /* the traced kernels walk their rays COLLECTIVELY: before every walk a 16x16 workgroup re-deals its rays to dense waves sorted by
                                       direction octant through LDS (csrc/experiments/frt_round4_walks.hpp: wg_trace): 1.65 vs 1.43 ms per frame
                                       (profiles/r4_experiments/collective_walks.md) */

/* FRT_PHASE_SPATIAL = the whole spatial stage. A strip renderer may issue it in two parts so that the halo exchange overlaps with
 * work: FRT_PHASE_SPATIAL_INNER (rows whose 10-row reuse neighbourhood lies inside the strip: needs nothing from a neighbour),
 * then, once the neighbours' temporal reservoirs have arrived, FRT_PHASE_SPATIAL_EDGE (the remaining rows + the continuations). */
enum { FRT_PHASE_GBUFFER = 1, FRT_PHASE_TEMPORAL = 2, FRT_PHASE_SPATIAL = 4, FRT_PHASE_POST = 8, FRT_PHASE_ALL = 15,
       FRT_PHASE_SPATIAL_INNER = 16, FRT_PHASE_SPATIAL_EDGE = 32 };

/* Per-pixel buffers (RenderTargets, src/renderer.rs:26-170; reservoirs src/passes/restir.rs:329-348) */
enum {
    FRT_BUF_GPOS = 0,        /* rgba32f  16 B/px, x2 ping-pong */
    FRT_BUF_GNORMAL = 1,     /* rgba32f  16 B/px, x2 */
    FRT_BUF_GALBEDO = 2,     /* rgba8    4 B/px, x2 */
    FRT_BUF_GMOTION = 3,     /* rg32f    8 B/px; index 0 = the last rendered frame (the reference has one motion texture); under
                                FRT_FLAG_OVERLAP_POST there are two slots internally and index 1 is the other one */
    FRT_BUF_RESERVOIR = 4,   /* 32 B/px, [0] temporal result, [1] spatial result */
    FRT_BUF_RAW = 5,         /* rgba16f  8 B/px */
    FRT_BUF_DISPLAY = 6,     /* rgba8    4 B/px */
    FRT_BUF_ACCUM = 7,       /* vec4f    16 B/px, x2 */
    FRT_BUF_CANDIDATE = 8    /* vec4f    16 B/px: (v1_pos, p_hat) of the temporal stage's fresh candidate path, T-trace -> T-merge (no reference
                                counterpart: restir.wgsl keeps it in registers between :825 and :826) */
};

typedef struct frt_stats {
    uint64_t rays_closest;    /* closest-hit rays issued (device-counted), since create/reset */
    uint64_t rays_any;        /* any-hit (shadow / visibility) rays issued */
    uint64_t frames;          /* frames rendered since create/reset */
    double ms_stage[4];       /* summed kernel time per stage (gbuffer, temporal, spatial, post); FRT_FLAG_TIMING only */
    uint64_t launches[4];     /* launches per stage */
    uint64_t rays_stage[4][2];/* per stage {closest, any}; post issues none */
    uint64_t halo_overflow;   /* strips: previous-frame reads (reprojection, history) outside own rows +- motion_halo_rows; 0 for a whole frame */
    double ms_merge;          /* summed T-merge kernel time (ms_stage[1] is T-trace); FRT_FLAG_TIMING only */
    uint64_t queue_overflow;  /* paths that found their continuation queue full and were finished in place */
    uint64_t queue_capacity;  /* current slots of the largest continuation queue (the spatial stage's first); the others are sized in proportion */
    uint64_t speculated_frames;       /* FRT_FLAG_PIPELINE: frames whose G-buffer + T-trace ran ahead and were adopted */
    uint64_t discarded_speculations;  /* ... and speculated work that did not match the next camera and was dropped */
    uint64_t queue_bytes;     /* device bytes of all continuation queues at the current capacity */
} frt_stats;

uint64_t frt_renderer_arena_bytes(uint32_t width, uint32_t height);
/* Renderer::new, src/renderer.rs:206. Uploads the scene replica to opts->device. */
frt_renderer* frt_renderer_create(const frt_scene* s, uint32_t width, uint32_t height, const frt_render_opts* opts);
void frt_renderer_destroy(frt_renderer* r);
/* Renderer::render, src/renderer.rs:349 — enqueue the four stages for one frame, then frame_count += 1 (:515). Asynchronous. */
int frt_renderer_render(frt_renderer* r, const frt_camera_uniform* cam);
/* Strip form: enqueue only `phases` (multi-GPU: a halo exchange sits between TEMPORAL and SPATIAL); frt_renderer_end_frame advances frame_count. */
int frt_renderer_render_phases(frt_renderer* r, const frt_camera_uniform* cam, int phases);
int frt_renderer_end_frame(frt_renderer* r);
/* PostParams.jitter (renderer.rs:14, :361-379): render(..., jitter) writes it before the post pass. set_jitter applies to the post
 * stages enqueued after it; render_jittered = set_jitter + render. (0, 0) — the shipped reference, camera.rs:202-203 — is the default.
 * Non-zero jitter makes post take bilinear radiance / albedo taps (post.wgsl:72-78, :97-109, :152-158); whole-frame renderers only. */
int frt_renderer_set_jitter(frt_renderer* r, float jitter_x, float jitter_y);
int frt_renderer_render_jittered(frt_renderer* r, const frt_camera_uniform* cam, float jitter_x, float jitter_y);
int frt_renderer_sync(frt_renderer* r);                       /* block until enqueued work is done */
/* Stream-level fence, no host wait: the renderer's stream (opts->stream) is ordered behind everything the renderer has enqueued on
 * its internal second stream (FRT_FLAG_PIPELINE). Call before touching buffers from frt_renderer_buffer_info on the caller's stream
 * (halo exchange, zero-copy views). */
int frt_renderer_fence(frt_renderer* r);
/* Orders the edge stream (frt_renderer_stream(r, 2)) behind the open frame's T-merge, now, with the event the renderer recorded behind T-merge anyway
 * (FRT_PHASE_SPATIAL_EDGE does the same later): for a caller that places a transfer of the T-merge's output IN that stream, in front of the edge rows'
 * launches (frt/rccl.py). Call after frt_renderer_render_phases(... TEMPORAL). A renderer without an edge stream: no-op. */
int frt_renderer_order_edge_stream(frt_renderer* r);
/* The streams the renderer enqueues on: which = 0 the main stream (opts->stream: T-merge, spatial, post — everything a halo exchange
 * reads), 1 the second stream of FRT_FLAG_PIPELINE (G-buffer + T-trace of the next frame), 2 the stream on which a strip renderer
 * under FRT_FLAG_PIPELINE launches FRT_PHASE_SPATIAL_EDGE's pixel kernels: a caller that receives halo rows orders THAT stream behind
 * the transfer before it issues the phase (frt/dist.py). Both equal stream 0 without the flag. */
void* frt_renderer_stream(const frt_renderer* r, int which);
uint32_t frt_renderer_frame_count(const frt_renderer* r);     /* renderer.frame_count, :198 */
int frt_renderer_reset(frt_renderer* r);                      /* frame_count = 0 only, as state.rs:152 / renderer.rs:346 (buffers keep their contents) */
int frt_renderer_clear(frt_renderer* r);                      /* back to the state right after create: zeroed targets, frame_count = 0, stats = 0 */
/* Read-back of post_processed_texture (state.rs:226-278) and of any other target; syncs first. index = ping-pong slot. */
int frt_renderer_read_display(frt_renderer* r, uint8_t* rgba8);
int frt_renderer_read_accum(frt_renderer* r, float* rgba32f);  /* the slot written by the last frame */
int frt_renderer_read_buffer(frt_renderer* r, int buf, int index, void* out);
/* Row-range copies to / from the host: rows [y0, y1) of a target, tightly packed (gathers of image strips, halo exchange through the host). */
int frt_renderer_read_rows(frt_renderer* r, int buf, int index, uint32_t y0, uint32_t y1, void* out);
int frt_renderer_write_rows(frt_renderer* r, int buf, int index, uint32_t y0, uint32_t y1, const void* in);
/* Device address / geometry of a target, for halo exchange and gathers by the caller (rows are contiguous, full-frame pitch). */
int frt_renderer_buffer_info(const frt_renderer* r, int buf, int index, void** device_ptr, uint32_t* bytes_per_pixel);
/* Rows this renderer computes per phase given its strip: out[0..1] gbuffer, [2..3] temporal, [4..5] spatial, [6..7] post */
int frt_renderer_phase_rows(const frt_renderer* r, uint32_t out[8]);
int frt_renderer_stats(frt_renderer* r, frt_stats* out);      /* syncs first */
/* Switch FRT_FLAG_TIMING on or off after creation (the per-stage HIP events cost ~25 us per frame: too much for a thin strip) */
int frt_renderer_set_timing(frt_renderer* r, int on);
/* Move instances in this renderer's scene replica between frames: the same arguments, checks and results as
 * frt_scene_set_instance_transforms, computed on the device by a transform kernel and a level-by-level refit. Asynchronous: enqueued behind every
 * kernel of the renderer that reads the scene and before the next frame's first one; a next frame's G-buffer + T-trace that already ran ahead
 * under the old geometry is dropped and redone. Accumulation and reservoirs are kept (moved objects ghost in temporal reuse until
 * frt_renderer_reset / _clear; motion vectors stay camera-only). FRT_ERR_STATE between the phases of an open frame; FRT_ERR_INVALID_ARG for a
 * renderer whose kernels walk a tree that is not refit (experiments build: FRT_FLAG_WALK_WIDE / _HBM with an 8-wide tree, the resident kernels). */
int frt_renderer_set_instance_transforms(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* m_colmajor16);
/* The same call with flags; flags == 0 is frt_renderer_set_instance_transforms.
 * FRT_TRANSFORM_DEVICE: ids (uint32[n], 4-byte aligned) and m_colmajor16 (float[16 n], 16-byte aligned) are device memory on the renderer's device, at
 * most 2^26 records. The call checks what the host can see (state, flags, that the pointers are device memory of this device inside an allocation that
 * holds n records from them on), enqueues everything on the renderer's main stream (frt_renderer_stream(r, 0): order it behind the producer of the
 * matrices first) and returns: no host copy of the ids or matrices and no wait for this call's work. The caller keeps the memory alive and unchanged
 * until that stream has passed the call. Ordering, state rules and refused renderers are the host form's, and so is the result, bit for bit: an id given
 * twice ends with its last matrix, world_to_object and flip come from the same cofactor formula in double, a registered light moves with its instance.
 * The checks of the data run on the device, all or nothing: a call with an id at or beyond the instance count, a non-finite matrix entry or a 3x3 whose
 * determinant is zero changes nothing of the replica (its kernels return at once; the refit that follows reproduces the same boxes) and adds one to a
 * counter that frt_renderer_transform_rejects reads; no kernel uses such an id as an index. The kernels read per-instance tables the renderer keeps on
 * the device (112 bytes + 4 per instance, uploaded at the first such call and again after an edit that changes what they restate), and the triangle
 * launch covers every triangle of the scene, since the host cannot know which instances move. From the first such call on the matrices live in a device
 * table: a later call that needs them on the host (the host form of this call, frt_renderer_set_mesh_vertices*, _add_instances, _remove_instances,
 * _register_*_light, _remove_lights) first waits for the main stream and reads the table back, once. */
#define FRT_TRANSFORM_DEVICE 1u
int frt_renderer_set_instance_transforms_ex(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* m_colmajor16, uint32_t flags);
/* Device-input transform calls this renderer has rejected since it was created (a bad id, a non-finite entry, a singular 3x3). Waits for the main stream. */
int frt_renderer_transform_rejects(frt_renderer* r, uint32_t* out);
/* Deform one mesh of this renderer's scene replica between two frames: arguments, checks and result of frt_scene_set_mesh_vertices, computed on the
 * device (the new vertices copied up, one kernel that rewrites the triangle slots and shading records of every instance of the mesh, the refit of
 * frt_renderer_set_instance_transforms). The inputs are copied during the call (the caller's arrays may be reused at once). Ordering, state rules
 * and refused renderers are those of frt_renderer_set_instance_transforms: asynchronous, behind every kernel that reads the scene, FRT_ERR_STATE
 * while a frame is open, a frame that ran ahead under the old geometry dropped and redone, accumulation, reservoirs and frame_count kept. Works on
 * a tree made by frt_renderer_rebuild_tree too, and later frt_renderer_set_instance_transforms calls transform the new vertices. */
int frt_renderer_set_mesh_vertices(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts);
/* The same call with flags; flags == 0 is frt_renderer_set_mesh_vertices.
 * FRT_DEFORM_RECOMPUTE_NORMALS: as frt_scene_set_mesh_vertices_ex, bit for bit, by a kernel with one thread per vertex that gathers through the mesh's
 * vertex -> corner adjacency. The adjacency is built on the host from the replica's indices at the first such call for a mesh (one read-back behind a
 * wait for the stream), kept on the device (4 (nverts + 1 + nidx) bytes per mesh) and follows frt_renderer_remove_meshes.
 * FRT_DEFORM_DEVICE: pos4 and attrs (if not NULL) are 16-byte aligned device memory on the renderer's device. The call checks what the host can see
 * (state, mesh id, vertex count, flags, that the pointers are device memory of this device inside an allocation that holds nverts records from them
 * on), enqueues everything on the renderer's main stream
 * (frt_renderer_stream(r, 0): order it behind the producer of the vertices first) and returns: no host copy of the vertices and no wait for this
 * call's work. The one wait a deformation of either kind may make is for the PREVIOUS deformation's small copies out of the pinned staging block
 * (its 64-byte instance records): a second call issued back to back blocks the host until the stream has reached the first one's copy, hence until
 * the work the stream was ordered behind for the first one has run. The caller keeps the memory alive
 * and unchanged until that stream has passed the call. The finiteness check runs on the device: a call with a non-finite position or attribute float
 * changes nothing of the replica (its kernels return at once; the refit that follows reproduces the same boxes) and adds one to a counter that
 * frt_renderer_deform_rejects reads. With attrs == NULL and FRT_DEFORM_RECOMPUTE_NORMALS no attribute is read from the caller. */
int frt_renderer_set_mesh_vertices_ex(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags);
/* Skin a mesh of this renderer's scene replica ("Skinning"): arguments, checks and results of frt_scene_set_mesh_skin and
 * frt_scene_set_mesh_pose, bit for bit, under the ordering and state rules of frt_renderer_set_mesh_vertices.
 * set_mesh_skin: joints and weights are copied during the call, through pinned memory, into device buffers kept per mesh (8 + 16 bytes per vertex); the
 * bind pose is a device-to-device copy of the replica's object-space positions as the stream finds them (16 bytes per vertex, no read-back). The buffers
 * follow frt_renderer_remove_meshes.
 * set_mesh_pose: flags are FRT_DEFORM_RECOMPUTE_NORMALS and FRT_DEFORM_DEVICE. Without FRT_DEFORM_DEVICE joint_mats is host memory: checked for finiteness
 * (FRT_ERR_INVALID_ARG) and copied during the call. With it, joint_mats is 16-byte aligned device memory of the renderer's device, 64 njoints bytes, under
 * the rules of the device form of frt_renderer_set_mesh_vertices_ex. One kernel skins the mesh into a scratch buffer of the renderer; from there the
 * vertices take the device-input route of frt_renderer_set_mesh_vertices_ex. What the host cannot see is rejected on the device as data: a non-finite
 * entry of a device palette (in a joint no vertex names too) and, for either kind of palette, a skinned coordinate that overflowed. Such a call changes
 * nothing of the replica and adds one to the counter frt_renderer_deform_rejects reads. */
int frt_renderer_set_mesh_skin(frt_renderer* r, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints);
/* ... with the skin mode (frt_scene_set_mesh_skin_ex: 0 or FRT_SKIN_DUAL_QUATERNION; set_mesh_skin is this call with flags 0). The mode is kept beside
 * the mesh's skin buffers, whose layout does not depend on it, and follows frt_renderer_remove_meshes with them. Every posing call of the renderer
 * (set_mesh_pose(_ex), set_mesh_poses, animate*, animate_cast*) poses a mesh in its mode, bit for bit what the scene's form gives: a call with a
 * dual-quaternion mesh runs one more kernel over the batch, which converts each vertex's four joint matrices in the lane; a call without one runs
 * exactly the launches it ran before the mode existed. The device rejects (deform_rejects) what the scene refuses: a zero column in a named joint and
 * a blend that cancels become non-finite coordinates, and a non-finite entry of a device palette is found by whichever skin kernel runs first. */
int frt_renderer_set_mesh_skin_ex(frt_renderer* r, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t flags);
int frt_renderer_set_mesh_pose(frt_renderer* r, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags);
/* Morph a mesh of this renderer's scene replica ("Morph targets"): arguments, checks and results of
 * frt_scene_set_mesh_morph_targets, frt_scene_set_mesh_morph_weights and frt_scene_set_mesh_pose_ex, bit for bit, under the ordering and state rules of
 * frt_renderer_set_mesh_pose.
 * set_mesh_morph_targets: the deltas are copied during the call, through pinned memory, into a device buffer kept per mesh (12 bytes per vertex and
 * target); the base is a device-to-device copy of the replica's object-space positions as the stream finds them (16 bytes per vertex, no read-back). The
 * buffer follows frt_renderer_remove_meshes.
 * set_mesh_morph_weights: flags are FRT_DEFORM_RECOMPUTE_NORMALS and FRT_DEFORM_DEVICE. Without FRT_DEFORM_DEVICE weights is host memory: checked for
 * finiteness (FRT_ERR_INVALID_ARG) and copied during the call. With it, weights is 4-byte aligned device memory of the renderer's device, 4 ntargets bytes,
 * under the rules of the device form of frt_renderer_set_mesh_vertices_ex. One kernel morphs the mesh into a scratch buffer of the renderer; from there the
 * vertices take the device-input route of frt_renderer_set_mesh_vertices_ex. What the host cannot see is rejected on the device as data: a non-finite
 * device weight (of a target whose deltas are all zero too) and, for either kind of weights, a morphed coordinate that overflowed. Such a call changes
 * nothing of the replica and adds one to the counter frt_renderer_deform_rejects reads.
 * set_mesh_pose_ex: the morph kernel writes a second scratch buffer, which frt_renderer_set_mesh_pose's kernel reads in the place of the skin's bind
 * pose. FRT_DEFORM_DEVICE covers both inputs: joint_mats (16-byte aligned) and morph_weights (4-byte aligned) are then both device memory. */
int frt_renderer_set_mesh_morph_targets(frt_renderer* r, uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets);
int frt_renderer_set_mesh_morph_weights(frt_renderer* r, uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags);
int frt_renderer_set_mesh_pose_ex(frt_renderer* r, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* Pose several meshes of this renderer's scene replica in one call ("Posing several meshes"): arguments, checks and results of
 * frt_scene_set_mesh_poses, bit for bit, under the ordering and state rules of frt_renderer_set_mesh_pose. mesh_ids is always host memory.
 * FRT_DEFORM_DEVICE covers joint_mats (16-byte aligned) and morph_weights (4-byte aligned), which are then both device memory of the renderer's device.
 * The number of kernel launches does not depend on n: one morph and/or one skin launch over the vertices of all n meshes into the renderer's scratch,
 * one validation, one copy-in, one normal and one triangle launch, then the scene-extent pass and the refit, once. The palette and the weights are
 * uploaded once. The call is atomic on the device as well: a non-finite entry of a device palette or weight vector, or a posed coordinate of ANY mesh
 * that overflowed, rejects the whole batch: no mesh of it changes, and the counter frt_renderer_deform_rejects reads goes up by one. */
int frt_renderer_set_mesh_poses(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* Device-input deformations this renderer has rejected since it was created (non-finite input). Waits for the main stream. */
int frt_renderer_deform_rejects(frt_renderer* r, uint32_t* out);

/* ---- animation ("Animation"): a rig is a node hierarchy, a joint list with inverse bind matrices, morph target defaults and
 * clips of keyframed channels, as a glTF document describes them. Evaluating clip c at time t gives the joint palette and the morph weights that
 * frt_scene_set_mesh_poses / frt_renderer_set_mesh_poses take. frt_rig_evaluate is the specification, on the host; frt_renderer_animate runs the same
 * text in one kernel on the renderer's device and gives the same bits.
 * The contract, f32 without contraction and without a hand-written fma (csrc/frt_animation.hpp, csrc/frt_math.hpp):
 *   Sampling a channel with key times times[0 .. K-1] at t: t <= times[0] gives the first key, t >= times[K-1] the last, t == times[k] key k, each as
 *   stored. Otherwise k is the largest index with times[k] <= t (binary search), dt = times[k+1] - times[k], u = (t - times[k]) / dt. Looping is the
 *   caller's (t % duration). STEP: key k. LINEAR (translation, scale, weights): a (1 - u) + b u per component. CUBICSPLINE (values stored per key as
 *   in-tangent, value, out-tangent): with u2 = u u, u3 = u2 u, h00 = (2 u3 - 3 u2) + 1, h10 = (u3 - 2 u2) + u, h01 = 3 u2 - 2 u3, h11 = u3 - u2:
 *   ((h00 v_k + (dt h10) b_k) + h01 v_k+1) + (dt h11) a_k+1 per component.
 *   Rotations (x, y, z, w): LINEAR is spherical. d = ((x0 x1 + y0 y1) + z0 z1) + w0 w1; d < 0 negates q1 and d. d > 0.9995: the component-wise mix,
 *   times 1 / sqrt of its own dot product. Otherwise th = acos(d) (a fixed polynomial, csrc/frt_animation.hpp: acosf_), q0 (sin((1 - u) th) / sin th) +
 *   q1 (sin(u th) / sin th), the quotient as a product with one reciprocal. CUBICSPLINE rotations are normalised after interpolation (between keys);
 *   STEP, key and rest rotations are used as given.
 *   Local matrix T R S: with x2 = x + x, y2, z2 alike and the nine products xx = x x2, xy = x y2, xz = x z2, yy = y y2, yz = y z2, zz = z z2,
 *   wx = w x2, wy = w y2, wz = w z2: columns (1 - (yy + zz), xy + wz, xz - wy) sx, (xy - wz, 1 - (xx + zz), yz + wx) sy, (xz + wy, yz - wx,
 *   1 - (xx + yy)) sz and (tx, ty, tz, 1). A path without a channel in the clip uses the node's rest value; a node given as a matrix uses its matrix
 *   and cannot be animated.
 *   global[n] = global[parent[n]] * local[n], a root's global is its local; a 4x4 product is column j = ((A.c0 b0j + A.c1 b1j) + A.c2 b2j) + A.c3 b3j.
 *   joint_mats[j] = global[joint_node[j]] * inverse_bind[j]. The transform of the node that carries a skinned mesh is not part of it (glTF): the
 *   instance transform places the character.
 *   Morph weights: the clip's weights channel sampled as ntargets components, or, in a clip without one, the default weights.
 * frt_rig_create: the description is copied. Nodes are given parents first (parents[n] is -1 or < n); rest_trs [10 nnodes] is translation xyz, rotation
 * xyzw, scale xyz per node; a node with has_matrix[n] != 0 takes matrices [16 n .. 16 n + 15] (column-major) instead (has_matrix and matrices may be
 * NULL: no such node). inverse_bind NULL: identities; default_weights NULL: zeros. A channel's values are [nkeys][width] (CUBICSPLINE:
 * [nkeys][3][width]) with width 3, 4, 3 or ntargets by path; a weights channel's node is not read. NULL with frt_last_error set: a count out of range
 * (nnodes 1 .. 2^20, njoints <= 65536, ntargets <= FRT_MAX_MORPH_TARGETS, neither joints nor targets), a parent that is not an earlier node, a joint
 * that is not a node, a channel on a node that is not a node or that is a matrix node, two channels of one clip for the same node and path or two
 * weights channels, an unknown path or interpolation, nkeys == 0, key times that are not finite and strictly increasing, a value that is not finite.
 * frt_rig_evaluate: joint_mats_out [16 njoints] (column-major), morph_weights_out [ntargets]; an output the rig has nothing for may be NULL.
 * FRT_ERR_INVALID_ARG: clip out of range, a time that is NaN or infinite. */
#define FRT_MAX_RIG_NODES 1024u         /* what frt_renderer_bind_rig takes: the kernel keeps every node's global matrix in LDS (64 bytes each) */
#define FRT_RIG_PATH_TRANSLATION 0u
#define FRT_RIG_PATH_ROTATION 1u
#define FRT_RIG_PATH_SCALE 2u
#define FRT_RIG_PATH_WEIGHTS 3u
#define FRT_RIG_STEP 0u
#define FRT_RIG_LINEAR 1u
#define FRT_RIG_CUBICSPLINE 2u
typedef struct frt_rig frt_rig;
typedef struct frt_rig_channel { uint32_t node, path, interpolation, nkeys; const float* times; const float* values; } frt_rig_channel;
typedef struct frt_rig_clip { const char* name; uint32_t nchannels; const frt_rig_channel* channels; } frt_rig_clip;
typedef struct frt_rig_desc {
    uint32_t nnodes; const int32_t* parents; const float* rest_trs; const uint8_t* has_matrix; const float* matrices;
    uint32_t njoints; const uint32_t* joint_nodes; const float* inverse_bind;
    uint32_t ntargets; const float* default_weights;
    uint32_t nclips; const frt_rig_clip* clips;
} frt_rig_desc;
frt_rig* frt_rig_create(const frt_rig_desc* desc);
/* The rig of a loaded glTF document (frt_model_load). The loader reads, beside the geometries: per primitive JOINTS_0 (u8 / u16) and WEIGHTS_0 (float or
 * normalized u8 / u16) in the geometry's vertex order, targets[*].POSITION and the mesh's default weights (JOINTS_1 and beyond: ignored with a warning;
 * target normals and tangents: ignored; sparse accessors: refused as everywhere); the nodes, stored parents first, with rest translation, rotation
 * (x, y, z, w), scale or their matrix; the skins (inverseBindMatrices absent: identities); the animations (outputs given as normalized integers are
 * converted by glTF's rule). frt_model_load fails for a cycle in the node graph, a joint that is not a node, sampler times that are not finite and
 * strictly increasing, an output count that is not input count x path width (x 3 for CUBICSPLINE); what is merely unsupported is skipped with a warning.
 * rig_counts: nodes, skins, animations. geometry_rig: {1 if the geometry has skin attributes, the skin of the node that carries its mesh or
 * 0xFFFFFFFF, its target count, its mesh's document index}. nodes_get: parents [N] (-1: a root, else a smaller stored index), rest_trs [10 N],
 * has_matrix [N], matrices [16 N], document_index [N] (the document's index of stored node i); any pointer may be NULL. skin_get: joint_nodes are
 * stored indices. channel_info: {node (stored index), path, interpolation, keys, values}. frt_rig_from_model: the rig of skin `skin_index`, or with
 * -1 a morph-only rig: every node, the skin's joints and inverse binds, the targets of the first geometry under that skin that has any, one clip per
 * animation. NULL with frt_last_error set when the skin is out of range or frt_rig_create refuses (a model with neither). */
int frt_model_rig_counts(const frt_model* m, uint32_t out[3]);
int frt_model_geometry_rig(const frt_model* m, uint32_t geo, uint32_t out[4]);
int frt_model_geometry_skin_get(const frt_model* m, uint32_t geo, uint16_t* joints4, float* weights4);
int frt_model_geometry_targets_get(const frt_model* m, uint32_t geo, float* deltas3, float* default_weights);
int frt_model_nodes_get(const frt_model* m, int32_t* parents, float* rest_trs, uint8_t* has_matrix, float* matrices, uint32_t* document_index);
int frt_model_skin_get(const frt_model* m, uint32_t skin, uint32_t* njoints, uint32_t* joint_nodes, float* inverse_bind);
int frt_model_animation_info(const frt_model* m, uint32_t anim, const char** name_out, uint32_t* nchannels);
int frt_model_channel_info(const frt_model* m, uint32_t anim, uint32_t channel, uint32_t out[5]);
int frt_model_channel_get(const frt_model* m, uint32_t anim, uint32_t channel, float* times, float* values);
frt_rig* frt_rig_from_model(const frt_model* m, int32_t skin_index);
void frt_rig_destroy(frt_rig* rig);
int frt_rig_counts(const frt_rig* rig, uint32_t counts[4]);      /* nodes, joints, targets, clips */
int frt_rig_clip_info(const frt_rig* rig, uint32_t clip, const char** name_out, float* duration_out);      /* duration: the largest last key time */
int frt_rig_evaluate(const frt_rig* rig, uint32_t clip, float time, float* joint_mats_out, float* morph_weights_out);
void frt_acosf(uint32_t n, const float* x, float* out);      /* TEST HOOK, not product API: the contract's acos of x [n], out[i] = acosf_(x[i]), so that a test can sweep it */
/* Animate meshes of this renderer's scene replica from a rig ("Animation").
 * bind_rig: the rig (topology, rest values, inverse binds, every clip's keys) is copied to the renderer's device once, through pinned memory, and a
 * palette of 4 njoints float4 and ntargets weights are allocated there; mesh_ids [n] is remembered. *binding_out names the binding from then on. The
 * rig may be destroyed afterwards. FRT_ERR_INVALID_ARG, nothing changed: more than FRT_MAX_RIG_NODES nodes, a mesh list frt_renderer_set_mesh_poses
 * would refuse for a palette of njoints joints (if the rig has joints) and ntargets weights (if it has targets) in device memory.
 * animate: asynchronous, between frames, on the main stream, under the ordering and state rules of frt_renderer_set_mesh_poses. One kernel (one
 * workgroup) evaluates `clip` at `time` into the binding's palette and weights, bit for bit what frt_rig_evaluate gives; then the call IS
 * frt_renderer_set_mesh_poses(r, n, mesh_ids, palette, njoints, weights, ntargets, flags | FRT_DEFORM_DEVICE): a rig with joints only skins, with
 * targets only morphs, with both morphs then skins. flags: FRT_DEFORM_RECOMPUTE_NORMALS. A palette entry or posed coordinate that overflowed rejects
 * on the device as any device palette does: nothing is applied and frt_renderer_deform_rejects counts one. Refused on the host with nothing enqueued
 * (FRT_ERR_INVALID_ARG): an unknown binding, clip out of range, a time that is not finite, an unknown flag bit, a mesh that no longer has the binding
 * the rig implies. read_rig_pose: waits for the main stream and copies the binding's palette [16 njoints] and weights [ntargets] as the last animate
 * left them (either may be NULL). unbind_rig: waits for the main stream and frees the binding's device memory; its number is given out again by a later bind_rig.
 * frt_renderer_remove_meshes renumbers a binding's meshes with the survivors and unbinds a binding that names a mesh that left. */
int frt_renderer_bind_rig(frt_renderer* r, const frt_rig* rig, const uint32_t* mesh_ids, uint32_t n, uint32_t* binding_out);
int frt_renderer_animate(frt_renderer* r, uint32_t binding, uint32_t clip, float time, uint32_t flags);
int frt_renderer_read_rig_pose(frt_renderer* r, uint32_t binding, float* joint_mats_out, float* morph_weights_out);
int frt_renderer_unbind_rig(frt_renderer* r, uint32_t binding);
/* Node animation ("Node animation"): a node's translation, rotation or scale channel moves the instance that hangs on it.
 * frt_rig_create_ex(desc, FRT_RIG_NODES_ONLY) also accepts a rig with neither joints nor targets; every other check is frt_rig_create's, and
 * frt_rig_create(desc) is frt_rig_create_ex(desc, 0). Node numbers are the caller's everywhere below: the rig remembers where frt_rig_create stored each
 * node (for a rig made from a model they are the stored node indices of frt_model_nodes_get).
 * frt_rig_evaluate_nodes is the specification, on the host: with G = global[nodes[k]] of the contract above, mats_out [16 k ..] = G, with `root` [16]
 * root * G, with `offsets` [16 n] (that) * offsets[k]: (root * G) * offset, the 4x4 product of the palette. A NULL root or offsets is no multiplication,
 * not a product with the identity (which would change the sign of a zero). FRT_ERR_INVALID_ARG: clip out of range (so a rig without clips cannot be
 * evaluated: give it one clip without channels for the rest pose), a time that is not finite, n == 0, a node that is not a node, a root or offsets
 * entry that is not finite, a null nodes or output.
 * frt_model_geometry_nodes: the stored indices, ascending, of the nodes whose mesh is the mesh of geometry `geo`; *count_out is their number, of which
 * the first `cap` are written (an OBJ model: none). frt_rig_from_model_nodes: every node, no joints, no targets, one clip per animation without its
 * weights channels, created with FRT_RIG_NODES_ONLY.
 * bind_rig_instances: the rig, instance_ids [n], the nodes' stored places, root and offsets (either may be NULL) are copied to the renderer's device
 * once, through pinned memory on the main stream, and n x 64 bytes are allocated for the matrices. The binding shares the numbers of frt_renderer_bind_rig
 * (the first free one is used again). FRT_ERR_INVALID_ARG, nothing changed: more than FRT_MAX_RIG_NODES nodes, n == 0 or n > FRT_MAX_RIG_INSTANCES, an
 * id at or beyond the instance count or given twice, a node that is not a node, a root or offsets entry that is not finite; and whatever
 * frt_renderer_set_instance_transforms refuses a renderer for. An instance with a registered light may be bound: the light moves with it.
 * animate_instances: asynchronous, between frames, on the main stream. One kernel (one workgroup) evaluates `clip` at `time` into the binding's
 * matrices, bit for bit frt_rig_evaluate_nodes; then the call IS frt_renderer_set_instance_transforms_ex(r, n, ids, matrices, FRT_TRANSFORM_DEVICE) on
 * the binding's device buffers: validated on the device, all or nothing (a node scaled to zero or an overflow rejects the call and
 * frt_renderer_transform_rejects counts one), refit, dropped speculation. Refused on the host with nothing enqueued: an unknown binding or a mesh binding
 * (and frt_renderer_animate refuses an instance binding), clip out of range, a time that is not finite.
 * read_rig_instances: waits for the main stream and copies the matrices [16 n] as the last animate_instances left them (zeros before the first).
 * frt_renderer_unbind_rig serves both kinds. frt_renderer_remove_instances (and _remove_lights) renumber a binding's instances with the survivors and
 * unbind a binding that names an instance that left. */
#define FRT_RIG_NODES_ONLY 1u
#define FRT_MAX_RIG_INSTANCES 65536u
frt_rig* frt_rig_create_ex(const frt_rig_desc* desc, uint32_t flags);
int frt_rig_evaluate_nodes(const frt_rig* rig, uint32_t clip, float time, uint32_t n, const uint32_t* nodes, const float* root16, const float* offsets16n, float* mats_out16n);
int frt_model_geometry_nodes(const frt_model* m, uint32_t geo, uint32_t cap, uint32_t* nodes_out, uint32_t* count_out);
frt_rig* frt_rig_from_model_nodes(const frt_model* m);
int frt_renderer_bind_rig_instances(frt_renderer* r, const frt_rig* rig, uint32_t n, const uint32_t* instance_ids, const uint32_t* nodes, const float* root16, const float* offsets16n, uint32_t* binding_out);
int frt_renderer_animate_instances(frt_renderer* r, uint32_t binding, uint32_t clip, float time);
int frt_renderer_read_rig_instances(frt_renderer* r, uint32_t binding, float* mats_out16n);
/* Animate a whole cast in one call ("Animating a cast"): entries [n], each a binding of either kind (frt_renderer_bind_rig,
 * frt_renderer_bind_rig_instances), a clip of its rig and a time, in any order. Asynchronous, between frames, on the main stream, under the ordering
 * and state rules of frt_renderer_animate. One kernel, one workgroup per entry, evaluates every entry into its binding's own buffers (what
 * read_rig_pose / read_rig_instances return) and into one buffer of the call. Then, inside one call frame:
 *   the instance half: every instance entry's matrices as ONE frt_renderer_set_instance_transforms_ex(.., FRT_TRANSFORM_DEVICE) over their
 *   concatenation, all or nothing (a singular or non-finite matrix anywhere applies none of it and counts one on transform_rejects);
 *   the mesh half: every mesh entry's meshes as ONE pose batch, each mesh under its own entry's palette and weights, all or nothing (a non-finite
 *   palette entry, weight or posed coordinate of any character applies none of it and counts one on deform_rejects); its triangles take the matrices
 *   the instance half left, from the device's matrix table, so the call does not wait for the stream;
 *   one scene-extent pass and one refit, if either half wrote a triangle.
 * The halves are independent, as two calls are. With every entry accepted the replica is, bit for bit, what frt_renderer_animate_instances for the
 * instance entries followed by frt_renderer_animate for the mesh entries leave (each group in any order). `flags`: FRT_DEFORM_RECOMPUTE_NORMALS or 0.
 * FRT_ERR_INVALID_ARG, nothing enqueued: n == 0 or above FRT_MAX_CAST_ENTRIES, entries == NULL, reserved != 0, unknown flag bits, an unknown or
 * unbound binding, a binding named twice, a mesh two mesh entries would pose, an instance two instance entries would move, a clip out of range, a
 * time that is not finite, a mesh that no longer has the skin or the morph targets its rig implies. FRT_ERR_STATE: as frt_renderer_animate. */
typedef struct frt_cast_entry { uint32_t binding, clip; float time; uint32_t reserved; } frt_cast_entry;      /* reserved must be 0 */
#define FRT_MAX_CAST_ENTRIES 4096u
int frt_renderer_animate_cast(frt_renderer* r, uint32_t n, const frt_cast_entry* entries, uint32_t flags);
/* Blending clips ("Blending clips"): a cross-fade between clips, for every animate call above. A SAMPLE is (clip, time, weight);
 * a BLEND is an ordered list of 1 .. FRT_MAX_BLEND_SAMPLES samples of one rig. Matrices do not blend and a palette has the hierarchy composed, so the
 * blend happens on a node's local translation, rotation and scale, in front of the local matrix; everything behind it is the contract of
 * frt_rig_evaluate, unchanged. The contract (csrc/frt_animation.hpp: rig_local_matrix_blend, rig_morph_weight_blend; f32, no contraction, no fma), for a
 * node that is not a matrix node, with the samples taken in the order given:
 *   A sample whose weight is 0 is skipped entirely. The first sample with a positive weight w gives the pose (T, R, S) as that clip sampled at that
 *   time gives it, without arithmetic, and W = w. Every later sample with a positive weight w and sampled pose (T_s, R_s, S_s):
 *   W = W + w; a = w / W; T = T (1 - a) + T_s a and S = S (1 - a) + S_s a per component; R = slerp(R, R_s, a), the slerp of the sampling rule above
 *   (the short way round, the mix above 0.9995). The local matrix is T R S of the result. A matrix node keeps its matrix.
 *   A path the clip of a sample has no channel for contributes the node's rest value, so two clips that animate different limbs each arrive at their
 *   share of the weight; there are no per-node masks.
 *   Morph weight c: the same running mix, r = r (1 - a) + r_s a, over the weight every sample gives by the rule above (a clip without a weights
 *   channel: the default weight).
 * So the weights need not sum to one, a blend of one sample (of any positive weight) is frt_rig_evaluate(clip, time) bit for bit, and so is a blend
 * whose other samples have weight 0, wherever they stand in the list.
 * frt_rig_evaluate_blend / frt_rig_evaluate_nodes_blend are the specification, on the host: outputs and the node arguments as frt_rig_evaluate /
 * frt_rig_evaluate_nodes take them. FRT_ERR_INVALID_ARG, nothing written: n == 0 or above FRT_MAX_BLEND_SAMPLES, samples == NULL, reserved != 0, a
 * clip out of range, a time or a weight that is not finite, a negative weight, no positive weight; and what the single-clip forms refuse.
 * frt_renderer_animate_blend / _animate_instances_blend / _animate_cast_blend are frt_renderer_animate / _animate_instances / _animate_cast with a
 * blend where those take (clip, time): the same kernels (the single-clip calls run them with a list of one sample of weight 1), the same launches,
 * rules and rejects, bit for bit the host forms; read_rig_pose / read_rig_instances return what they wrote. The samples of a one-binding call are a
 * kernel argument; those of a cast lie in samples [nsamples], entry k naming samples [first_sample .. first_sample + num_samples), and are uploaded
 * with the entry table in the one staged copy. Refused on the host with nothing enqueued: what the single-clip call refuses, what
 * frt_rig_evaluate_blend refuses of a list, and for a cast nsamples == 0, an entry whose range is empty, longer than FRT_MAX_BLEND_SAMPLES or not
 * inside nsamples. Ranges may overlap or leave samples unused. */
#define FRT_MAX_BLEND_SAMPLES 8u
typedef struct frt_clip_sample { uint32_t clip; float time, weight; uint32_t reserved; } frt_clip_sample;      /* reserved must be 0 */
int frt_rig_evaluate_blend(const frt_rig* rig, uint32_t n, const frt_clip_sample* samples, float* joint_mats_out, float* morph_weights_out);
int frt_rig_evaluate_nodes_blend(const frt_rig* rig, uint32_t n, const frt_clip_sample* samples, uint32_t nnodes, const uint32_t* nodes, const float* root16, const float* offsets16n, float* mats_out16n);
int frt_renderer_animate_blend(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_sample* samples, uint32_t flags);
int frt_renderer_animate_instances_blend(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_sample* samples);
typedef struct frt_cast_blend_entry { uint32_t binding, first_sample, num_samples, reserved; } frt_cast_blend_entry;      /* reserved must be 0 */
int frt_renderer_animate_cast_blend(frt_renderer* r, uint32_t n, const frt_cast_blend_entry* entries, uint32_t nsamples, const frt_clip_sample* samples, uint32_t flags);
/* Layering clips ("Layering clips"): wave with the arm while the legs walk, lean on top of whatever plays, fade a layer over a
 * part of the skeleton. A LAYER is a clip at a time with a weight, a mode and, optionally, a mask; a call takes an ordered list of 1 .. FRT_MAX_LAYERS
 * layers of one rig. A MASK is one float in [0, 1] per node of the rig, in the caller's node order; a call sees nmasks <= FRT_MAX_RIG_MASKS of them
 * as masks [nmasks][nnodes] and a layer names one by index, FRT_LAYER_NO_MASK meaning 1 everywhere. As with a blend, the layers meet on a node's
 * local translation, rotation and scale, in front of the local matrix; everything behind it is the contract of frt_rig_evaluate, unchanged.
 * frt_clip_sample and every call above keep their meaning and their refusals. The contract (csrc/frt_animation.hpp: rig_local_matrix_layers,
 * rig_morph_weight_layers, rig_qmul; f32, no contraction, no fma), for a node n that is not a matrix node (a matrix node keeps its matrix), the layers
 * folded in the order given into ONE running pose (T, R, S) with an accumulated blend weight W:
 *   Layer 0 is the base: its mode is BLEND, it has no mask and its weight is positive. The pose is that clip sampled at that time, without
 *   arithmetic, and W = weight. So every node has a base.
 *   Every later layer: m = 1 or masks[mask][n], e = weight * m. If !(e > 0) the layer is skipped for this node and nothing is sampled. Otherwise
 *   X = (X.t, X.q, X.s) is the layer's clip sampled at its time and
 *     FRT_LAYER_BLEND: the blend's rule with e for w: W = W + e, a = e / W, T = T (1 - a) + X.t a and S likewise per component, R = slerp(R, X.q, a).
 *     FRT_LAYER_OVERRIDE (weight <= 1): a = e. At a >= 1 the pose becomes X without arithmetic; otherwise the same mix and slerp by a. W is unchanged.
 *     FRT_LAYER_ADDITIVE: Y is ref_clip sampled at ref_time. T = T + e (X.t - Y.t) and S = S + e (X.s - Y.s) per component; D = conj(Y.q) * X.q,
 *     R = R * slerp((0, 0, 0, 1), D, e), the quaternion product with every product and sum written once in a fixed order (rig_qmul). R is not
 *     renormalised, a weight above 1 is allowed (it extrapolates), W is unchanged.
 *   The local matrix is T R S of the result.
 *   Morph weight c: the weights every layer's clip gives, folded the same way with e = weight (masks do not apply to targets): BLEND the running mix,
 *   OVERRIDE the mix by the weight or the layer's own value at weight >= 1, ADDITIVE r + weight (x - x_ref). A layer with FRT_LAYER_KEEP_MORPH in its
 *   flags leaves the morph weights alone.
 * So a list of BLEND layers without masks is frt_rig_evaluate_blend of the same (clip, time, weight) rows bit for bit; an all-ones mask is no mask;
 * a layer of weight 0, or under an all-zero mask, anywhere but first is as good as absent; and an OVERRIDE layer of weight 1 under a 0 / 1 mask
 * replaces exactly the masked nodes' poses.
 * frt_rig_evaluate_layers / frt_rig_evaluate_nodes_layers are the specification, on the host: outputs and the node arguments as the _blend forms take
 * them. FRT_ERR_INVALID_ARG, nothing written: n == 0 or above FRT_MAX_LAYERS, layers == NULL, an unknown mode or flag bit, a clip out of range, on an
 * ADDITIVE layer a ref_clip out of range (every other mode: ref_clip and ref_time must be 0), a time, reference time or weight that is not finite, a
 * negative weight, an OVERRIDE weight above 1, a mask index that is neither FRT_LAYER_NO_MASK nor below nmasks, a layer 0 that is not (BLEND, no mask,
 * weight > 0) or that has FRT_LAYER_KEEP_MORPH; nmasks above FRT_MAX_RIG_MASKS, masks == NULL with nmasks > 0, a mask value that is not finite or
 * outside [0, 1]; and what the _blend forms refuse of their other arguments.
 * frt_renderer_set_rig_masks gives a binding of either kind its masks: they are uploaded in the rig's stored node order by a staged asynchronous
 * copy on the main stream, replace the previous set (nmasks == 0 clears it), and take effect in stream order, so a call placed between two animate
 * calls needs no wait. Refused with nothing changed: an unknown binding, and the mask refusals above.
 * frt_renderer_animate_layers / _animate_instances_layers / _animate_cast_layers are frt_renderer_animate_blend / _animate_instances_blend /
 * _animate_cast_blend with layers where those take samples: kernels of the same three phases whose first phase folds the layers in registers, the
 * same launches, rules and rejects behind the kernel, bit for bit the host forms under the binding's masks. The layers of a one-binding call are a
 * kernel argument; those of a cast lie in layers [nlayers], entry k naming layers [first_layer .. first_layer + num_layers), each entry under its own
 * binding's masks. Refused on the host with nothing enqueued: what the _blend call refuses of its other arguments, what frt_rig_evaluate_layers
 * refuses of a list (seen with the binding's mask count), and for a cast nlayers == 0, an entry whose range is empty, longer than FRT_MAX_LAYERS or
 * not inside nlayers. */
#define FRT_MAX_LAYERS 8u
#define FRT_MAX_RIG_MASKS 16u
#define FRT_LAYER_NO_MASK 0xFFFFFFFFu
enum { FRT_LAYER_BLEND = 0, FRT_LAYER_OVERRIDE = 1, FRT_LAYER_ADDITIVE = 2 };
#define FRT_LAYER_KEEP_MORPH 1u     /* flags: the layer leaves the morph weights alone */
typedef struct frt_clip_layer {
    uint32_t clip; float time, weight; uint32_t mask;
    uint32_t mode, ref_clip; float ref_time; uint32_t flags;
} frt_clip_layer;   /* 32 bytes */
int frt_rig_evaluate_layers(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, float* joint_mats_out, float* morph_weights_out);
int frt_rig_evaluate_nodes_layers(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t nnodes, const uint32_t* nodes, const float* root16, const float* offsets16n, float* mats_out16n);
int frt_renderer_set_rig_masks(frt_renderer* r, uint32_t binding, uint32_t nmasks, const float* masks);
int frt_renderer_animate_layers(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_layer* layers, uint32_t flags);
int frt_renderer_animate_instances_layers(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_layer* layers);
typedef struct frt_cast_layers_entry { uint32_t binding, first_layer, num_layers, reserved; } frt_cast_layers_entry;      /* reserved must be 0 */
int frt_renderer_animate_cast_layers(frt_renderer* r, uint32_t n, const frt_cast_layers_entry* entries, uint32_t nlayers, const frt_clip_layer* layers, uint32_t flags);
/* Inverse kinematics ("Inverse kinematics"): goals on a rig, behind the layers. A GOAL acts on the GLOBAL matrices of the rig,
 * in the rig's model space: for a mesh binding the space of the palette, for an instance binding the space in front of `root` and the offsets (the
 * caller maps world space into it). Goals act after the layers have been folded and the hierarchy walked, and before joints or instances read the
 * globals; they are applied in list order, each seeing what the earlier ones left. 0 .. FRT_MAX_RIG_GOALS of them, of three kinds; node numbers are
 * the caller's. The contract (csrc/frt_ik.hpp: ik_arc, ik_about, ik_two_bone, ik_aim; f32, no contraction, no fma, one text for host and kernel):
 *   arc(u, v), unit vectors: q = (cross(u, v), 1 + dot(u, v)) * rsqrt(|q|^2); if 1 + dot < FRT_IK_ARC_EPS, the half turn about cross(u, e), e the
 *   coordinate axis of u's smallest |component|. about(p, q): the m4 whose 3x3 is q's rotation and whose last column is p - R p.
 *   A target record is (target xyz, weight w, pole xyz, pole flag). A goal whose record has a word that is not finite, or w outside (0, 1], is
 *   SKIPPED: nothing is written, as if the goal were absent.
 *   FRT_GOAL_TWO_BONE (root, mid, tip; mid a strict descendant of root, tip of mid; nodes between them are carried rigidly): A, B, C the origins
 *   (last columns) of their globals. Te = C + w (T - C), at w == 1 T itself. lab = |B - A|, lcb = |C - B|, d = |Te - A|; skipped unless all three
 *   are > 0. dir = (Te - A) / d, lat = min(max(d, |lab - lcb|), lab + lcb). side = P - A with a pole (flag != 0), else B - A; nrm = cross(dir, side);
 *   unless dot(nrm, nrm) > FRT_IK_PLANE_EPS dot(side, side), a goal with a pole tries side = B - A, and one that still fails is skipped (a straight
 *   limb without a usable pole has no bend plane). perp = cross(nrm / |nrm|, dir); c = (lab^2 + lat^2 - lcb^2) / (2 lab lat) clamped to [-1, 1],
 *   s = sqrt(max((lat + (lcb - lab)) ((lab + lcb) - lat) (lat + (lab - lcb)) ((lab + lcb) + lat), 0)) / (2 lab lat) (the sine from the triangle's
 *   area: sqrt(1 - c c) would lose half the digits where c = 1, and a clamped lat makes this form exactly 0); B' = A + lab (c dir + s perp), C' = A + lat dir. Da = about(A, arc(norm(B - A), norm(B' - A))), C1 = Da C,
 *   Db = about(B', arc(norm(C1 - B'), norm(C' - B'))). Every node of subtree(mid) takes G = mul(mul(Db, Da), G), every other node of subtree(root)
 *   G = mul(Da, G).
 *   FRT_GOAL_AIM (root = the node, mid = tip = 0; axis: a non-zero local direction): O the origin of G[node], cur = norm(G[node]'s 3x3 * axis),
 *   want = norm(T - O); skipped when either length is not > 0. q = arc(cur, want), for w < 1 rig_slerp((0, 0, 0, 1), q, w); every node of
 *   subtree(node) takes G = mul(about(O, q), G). The pole words of an AIM record are 0.
 *   FRT_GOAL_CHAIN ("Chain IK"; csrc/frt_ik.hpp: ik_chain_target, ik_chain_step): cyclic coordinate descent over the parent path c_0 = root, ...,
 *   c_K = tip (tip a strict descendant of root; every node of the path is a joint of the chain; 2 <= K + 1 <= FRT_IK_CHAIN_MAX_NODES). `mid` is
 *   the number of sweeps S, 1 <= S <= FRT_IK_CHAIN_MAX_SWEEPS; `axis` is unused and not kept; `reserved` is 0. P_j the origin of G[c_j], D_j the
 *   identity, j = 0 .. K. Te = P_K + w (T - P_K), at w == 1 T itself, taken once. For s = 0 .. S - 1 and, within a sweep, k = K - 1 down to 0:
 *   e = P_K - P_k, t = Te - P_k; if sqrt(dot(e, e)) > 0 and sqrt(dot(t, t)) > 0: R = about(P_k, arc(norm(e), norm(t))), P_j = R P_j for j > k,
 *   D_j = mul(R, D_j) for j >= k; otherwise the step changes nothing. No convergence test, no early exit: the cost is S K steps. Every node n of
 *   subtree(root) takes G = mul(D_j, G), c_j the deepest chain node whose subtree holds n, the tip's own subtree D_(K-1): the tip is an end
 *   effector and does not turn itself. The pole words are ignored (but a record with a non-finite one is skipped, as above). Both caps are design
 *   constants, not measurements: 32 nodes is what half a wave's lanes hold.
 *   FRT_IK_PLANE_EPS and FRT_IK_ARC_EPS are design constants of the contract, not measurements.
 * frt_rig_evaluate_layers_ik / frt_rig_evaluate_nodes_layers_ik are the specification, on the host: the layered calls with goals [ngoals] and their
 * targets [ngoals]; ngoals == 0 is the layered call bit for bit. FRT_ERR_INVALID_ARG, nothing written: what the layered call refuses; ngoals above
 * FRT_MAX_RIG_GOALS; a null array with ngoals > 0; an unknown kind; reserved != 0; a node out of range; a mid that is not a strict descendant of
 * root or a tip that is not one of mid; an AIM axis that is not finite or is zero, or AIM mid / tip != 0; a target word that is not finite, a
 * weight outside [0, 1] (0: the goal is skipped), a pole flag other than 0 or 1, a non-zero pole word on an AIM record; a CHAIN tip that is not
 * a strict descendant of root, a path of more than FRT_IK_CHAIN_MAX_NODES nodes, sweeps (`mid`) outside 1 .. FRT_IK_CHAIN_MAX_SWEEPS.
 * Goals and targets are state of a binding of either kind, as masks are. frt_renderer_set_rig_goals uploads the definitions (staged, asynchronous,
 * on the main stream), replaces the previous set (ngoals == 0 clears it) and resets every target to weight 0, so new goals do nothing until
 * targets arrive. frt_renderer_set_rig_goal_targets is one asynchronous copy of ngoals records (ngoals: the binding's goal count) into the
 * binding's targets: from host memory (flags 0) checked as above and staged; with FRT_GOAL_TARGETS_DEVICE from device memory of the renderer's
 * device (16-byte aligned, ordered by the caller on the main stream or on a stream the main stream has been made to wait for, alive until the
 * stream has passed the call), unseen by the host: the kernel then applies the skip rule above to each record, and any other pole flag than 0
 * uses the pole. Both calls take effect in stream order, without a wait. Refused with nothing enqueued: an unknown binding, what the host form
 * refuses of goals or host targets, a count that is not the binding's, unknown flag bits, a pointer that is not such device memory.
 * Only frt_renderer_animate_layers / _animate_instances_layers / _animate_cast_layers apply a binding's goals (a single clip under goals is a stack
 * of one layer): their results are the _ik host forms' bit for bit. frt_renderer_animate, _animate_blend, _animate_instances,
 * _animate_instances_blend and the plain and blended casts ignore them. */
#define FRT_MAX_RIG_GOALS 16u
enum { FRT_GOAL_TWO_BONE = 0, FRT_GOAL_AIM = 1 };
#define FRT_GOAL_CHAIN 2u
#define FRT_IK_CHAIN_MAX_NODES 32u
#define FRT_IK_CHAIN_MAX_SWEEPS 16u
#define FRT_IK_PLANE_EPS 1e-12f
#define FRT_IK_ARC_EPS 1e-6f
#define FRT_GOAL_TARGETS_DEVICE 1u
typedef struct frt_rig_goal { uint32_t kind, root, mid, tip; float axis[3]; uint32_t reserved; } frt_rig_goal;            /* 32 bytes; AIM: root = node, mid = tip = 0; CHAIN: mid = sweeps */
typedef struct frt_rig_goal_target { float target[3], weight, pole[3], pole_flag; } frt_rig_goal_target;                  /* 32 bytes; pole_flag 0 or 1 */
int frt_rig_evaluate_layers_ik(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals, const frt_rig_goal* goals, const frt_rig_goal_target* targets, float* joint_mats_out, float* morph_weights_out);
int frt_rig_evaluate_nodes_layers_ik(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals, const frt_rig_goal* goals, const frt_rig_goal_target* targets, uint32_t nnodes, const uint32_t* nodes, const float* root16, const float* offsets16n, float* mats_out16n);
int frt_renderer_set_rig_goals(frt_renderer* r, uint32_t binding, uint32_t ngoals, const frt_rig_goal* goals);
int frt_renderer_set_rig_goal_targets(frt_renderer* r, uint32_t binding, uint32_t ngoals, const frt_rig_goal_target* targets, uint32_t flags);
/* Edit what this renderer's scene replica looks like between two frames: arguments, checks and results of the frt_scene_* calls
 * of the same names, bit for bit. set_materials, set_light_emission and set_texture are copies into the replica's tables (a texture: one 4 MiB
 * host-to-device copy); set_instance_materials is one kernel that stores the changed word of every affected shading and instance record. The inputs
 * are copied during the call. Ordering and state rules are those of frt_renderer_set_instance_transforms: asynchronous, behind every kernel that
 * reads the scene and before the next frame's first one, FRT_ERR_STATE while a frame is open, a next frame's G-buffer + T-trace that ran ahead under
 * the old values dropped and redone. Accumulation, reservoirs, frame_count and the tree are kept: an edited surface converges to its new look only
 * through frt_renderer_reset / _clear (until then temporal reuse and the accumulated frame still carry the old one). No tree is involved, so every
 * renderer takes these calls, those of the experiments build that the other edit calls refuse included. frt_renderer_pick and _trace_closest
 * report the material of the instance record, so they see set_instance_materials at once. */
int frt_renderer_set_materials(frt_renderer* r, uint32_t n, const uint32_t* ids, const frt_material* materials);
int frt_renderer_set_instance_materials(frt_renderer* r, uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids);
int frt_renderer_set_light_emission(frt_renderer* r, uint32_t light, const float color[3], float intensity);
int frt_renderer_set_texture(frt_renderer* r, int kind, uint32_t layer, const uint8_t* rgba8_1024x1024);
/* Build a new quad tree over the triangle slots as they are on the device now, i.e. after any number of frt_renderer_set_instance_transforms calls, whose
 * refit keeps the topology and so loses quality after large moves ("Rebuild"): Morton order, leaves of two adjacent slots, a binary
 * radix tree folded into quad nodes, boxes by the refit kernel; all on the device, into a second set of buffers that is swapped in only on success. Hits are
 * defined without reference to any tree, so pixels, ray counts, accumulation, reservoirs and frame_count are untouched. SYNCHRONOUS, unlike the instance
 * update: the per-level node counts and the stack need come back to the host, so the call returns when the new tree is in place; call it between frames.
 * The first call allocates the extra device memory (DESIGN.md gives the size). Afterwards frt_renderer_read_scene selectors 10 and 13 return the new tree
 * and later frt_renderer_set_instance_transforms calls refit it. The pair tree and its quantised form are NOT rebuilt (the product's kernels walk the quad
 * nodes only): later refits skip them and selector 15 returns FRT_ERR_STATE. The host frt_scene gets no rebuild: its tree stays the host build's.
 * Errors, nothing changed in each case: FRT_ERR_STATE between the phases of an open frame; FRT_ERR_INVALID_ARG for a renderer whose kernels walk a tree this
 * call does not make (experiments build: the renderers frt_renderer_set_instance_transforms refuses, and the kernel families that walk the pair tree);
 * FRT_ERR_LIMIT if the finished tree needs more than 31 traversal-stack entries (computed on the device, checked before the swap). */
int frt_renderer_rebuild_tree(frt_renderer* r);
/* The same call with a choice of tree ("Refined rebuild"). FRT_REBUILD_MORTON is frt_renderer_rebuild_tree, byte for byte.
 * FRT_REBUILD_SAH keeps the Morton order and the leaves of two adjacent slots but builds the binary tree above them by parallel locally-ordered
 * clustering on the surface area of merged boxes and folds it into quad nodes largest-area-first, as the host build folds; same contract, same
 * errors, deterministic. Its first call allocates 50 B per triangle more and the call takes about 1.5x as long. A refined tree that does not fit the 31 traversal-stack entries, or
 * whose clustering passes its iteration bound, is replaced inside the call by the Morton tree (frt_renderer_tree_stats then reports origin 1), so
 * FRT_ERR_LIMIT means that the Morton tree does not fit either. Any other mode: FRT_ERR_INVALID_ARG, nothing changed. */
#define FRT_REBUILD_MORTON 0
#define FRT_REBUILD_SAH 1
int frt_renderer_rebuild_tree_ex(frt_renderer* r, uint32_t mode);
/* The quad tree of this renderer's replica: stats[4] = quad nodes, deepest traversal stack, levels, origin (0 host build, 1 device Morton tree,
 * 2 device refined tree) */
int frt_renderer_tree_stats(frt_renderer* r, uint32_t stats[4]);
/* The last rebuild call that reached the device: stats[4] = mode asked for, clustering iterations run (FRT_REBUILD_SAH), why the Morton tree was
 * built instead (0 it was not, 1 iteration bound, 2 traversal stack), KiB of device memory the refined mode has added. Zeros before any rebuild. */
int frt_renderer_rebuild_stats(frt_renderer* r, uint32_t stats[4]);
/* Read the device replica back (syncs first), in the layout of frt_scene_get: 2 materials, 3 lights, 4 attributes, 5 indices, 6 mesh infos
 * (frt_renderer_pool_counts gives their counts), 10 quad nodes (frt_renderer_tree_stats gives the count), 13 triangle slots, 15 pair nodes (FRT_ERR_STATE
 * after frt_renderer_rebuild_tree), 16 device instance records, 17 shading records; and 18: the decoded normal of every vertex (16 B: xyz, 0; indexed
 * as the attributes), which frt_renderer_add_instances builds its shading records from. */
int frt_renderer_read_scene(frt_renderer* r, int which, void* out);
/* counts[4]: triangles, instances, materials, lights of the replica AS IT IS NOW (what sizes the arrays of frt_renderer_read_scene). */
int frt_renderer_scene_counts(frt_renderer* r, uint32_t counts[4]);
/* frt_scene_add_instances / _remove_instances on this renderer's scene replica, on the device: the same arguments, checks and results.
 * The new triangles, shading records, instance records and id -> slot table are written out of place and the call ends with the device tree rebuild of
 * frt_renderer_rebuild_tree_ex in `rebuild_mode` (FRT_REBUILD_MORTON, FRT_REBUILD_SAH); all of it enters the replica together, on success only. Synchronous,
 * between frames. Afterwards selectors 2, 3, 16 and 17 of frt_renderer_read_scene equal, byte for byte, those of a freshly built scene with the same instance
 * list, selector 13 holds the same triangle records in the device tree's order, and every frame equals that scene's bit for bit. A next frame's G-buffer +
 * T-trace that ran ahead is dropped and redone; accumulation, reservoirs and frame_count are kept (the change ghosts until frt_renderer_reset / _clear).
 * The host frt_scene is not changed. Device buffers grow geometrically and are never shrunk; the per-pixel arena is untouched.
 * Errors, nothing changed in each case: those of the host calls (the scene is always "built"); FRT_ERR_STATE between the phases of an open frame;
 * FRT_ERR_INVALID_ARG for an unknown rebuild_mode or a renderer frt_renderer_rebuild_tree refuses; FRT_ERR_LIMIT if the new tree needs more than 31
 * traversal-stack entries. FRT_ERR_HIP leaves the renderer failed (frt_renderer_clear). */
int frt_renderer_add_instances(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* m_colmajor16, uint32_t rebuild_mode);
int frt_renderer_remove_instances(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode);
/* New meshes, materials, texture layers and lights for this renderer's scene replica between frames. The specification is the host
 * route on a built scene: frt_scene_add_mesh / _add_material / _add_texture / _add_light / _register_*_light followed by frt_scene_build. After any sequence
 * of these calls and the edits above the replica holds what a scene built from scratch with the same builder calls holds: ids, flattened triangle ids,
 * mesh infos and offsets, material and light records, layer numbering; frt_renderer_read_scene selectors 2 - 6, 16 and 17 equal it byte for byte, 13 as a
 * set of records, and every frame equals that scene's bit for bit. Everything is validated before anything is applied, a refused call changes nothing,
 * n == 0 is FRT_OK (the add calls: the current count), FRT_ERR_STATE while a frame is open, a next frame's G-buffer + T-trace that ran ahead is dropped and
 * redone, accumulation, reservoirs and frame_count are kept. The inputs are copied during the call. The new ids are accepted at once by
 * frt_renderer_add_instances, _set_mesh_vertices, _set_materials, _set_instance_materials, _set_light_emission and _set_texture; the caller passes the new
 * light count in frt_camera_uniform.num_lights from the next frame on. What was added can be taken out again: frt_renderer_remove_* below.
 * add_meshes / _materials / _texture / _lights add no triangle: no rebuild, asynchronous on the renderer's stream; they wait for the stream only when a
 * capacity grows (capacities at least double, texture arrays grow by max(4, count / 2) layers, and are never shrunk). Returns: the id of the first new
 * mesh / material, the layer id, the index of the first new light (lights as frt_scene_add_light takes them: no instance, no link).
 * register_quad_light / _sphere_light: what frt_scene_register_quad_light / _sphere_light make: a new emissive material, a new instance of `mesh_id` and
 * a new light record linked to it, then the device rebuild of frt_renderer_add_instances in `rebuild_mode` (synchronous). Returns the light index. The
 * instance then behaves as any registered light's: frt_renderer_set_instance_transforms moves the light, _set_light_emission edits it, _remove_instances
 * and _set_instance_materials refuse it.
 * FRT_ERR_INVALID_ARG: a null pointer with n > 0; nverts == 0; nidx == 0 or not a multiple of 3; an index >= nverts; a non-finite position or attribute
 * float; a material that fails frt_scene_build's check against the replica's layers and lights as they are; a light with a non-finite field or
 * area <= 0; kind not 0 or 1; mesh_id out of range, a non-finite or singular matrix, an unknown rebuild_mode. FRT_ERR_LIMIT: vertex or index totals
 * beyond 32 bits, more than 65,535 materials, a 65,535th texture layer, a failed allocation, a new tree beyond 31 traversal-stack entries. */
typedef struct frt_mesh_data { const float* pos4; const frt_vertex_attr* attrs; const uint32_t* idx; uint32_t nverts, nidx; } frt_mesh_data;
int frt_renderer_add_meshes(frt_renderer* r, uint32_t n, const frt_mesh_data* meshes);
int frt_renderer_add_materials(frt_renderer* r, uint32_t n, const frt_material* materials);
int frt_renderer_add_texture(frt_renderer* r, int kind /*0 colour (sRGB), 1 data*/, const uint8_t* rgba8_1024x1024);
int frt_renderer_add_lights(frt_renderer* r, uint32_t n, const frt_light* lights);
int frt_renderer_register_quad_light(frt_renderer* r, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity, uint32_t rebuild_mode);
int frt_renderer_register_sphere_light(frt_renderer* r, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity, uint32_t rebuild_mode);
/* counts[6]: meshes, vertices, indices, colour layers, data layers of the replica AS IT IS NOW (with frt_renderer_scene_counts what sizes the arrays of
 * frt_renderer_read_scene), and the calls above that had to grow a capacity so far. */
int frt_renderer_pool_counts(frt_renderer* r, uint32_t counts[6]);
/* frt_scene_remove_materials / _meshes / _lights / _texture on this renderer's scene replica, on the device: the same arguments, checks
 * and refusals, under the contract of the add calls above: after any sequence of these calls and every other edit the replica holds what a scene built from
 * scratch with the surviving builder calls holds (frt_renderer_read_scene selectors 2 - 6, 16 and 17 byte for byte, 13 as a set of records, every frame bit
 * for bit); everything is validated first, a refused call changes nothing, n == 0 is FRT_OK, FRT_ERR_STATE while a frame is open; a next frame's G-buffer +
 * T-trace that ran ahead is dropped and redone; accumulation, both reservoir buffers and frame_count are kept. Counts move (frt_renderer_scene_counts,
 * _pool_counts), capacities are never shrunk. The removed ids' successors are accepted at once by every other call under their new ids; the caller passes
 * the new light count in frt_camera_uniform.num_lights from the next frame on.
 * Per-pixel history: the one id a pixel keeps between frames is the material id in FRT_BUF_GPOS.w, which temporal reprojection compares. Whenever materials
 * are renumbered (remove_materials; remove_lights of a registered light) that word is renumbered in every G-buffer set the renderer owns: a hit's id follows,
 * an id that left becomes 65535.0 (no valid id: such a pixel restarts its reservoir), the miss word -1 stays. Nothing else per pixel changes.
 * remove_materials, _meshes, _texture, and remove_lights of lights that have no instance add no triangle work and are only enqueued on the renderer's stream
 * (remove_lights and remove_texture wait for the device once: their checks read the material table back). remove_lights of a registered light removes its
 * instance as frt_renderer_remove_instances does, with the device rebuild in `rebuild_mode`, and is synchronous; a tree that is refused (FRT_ERR_LIMIT)
 * leaves everything as it was. FRT_ERR_INVALID_ARG also for an unknown rebuild_mode. FRT_ERR_HIP leaves the renderer failed (frt_renderer_clear). */
int frt_renderer_remove_materials(frt_renderer* r, uint32_t n, const uint32_t* ids);
int frt_renderer_remove_meshes(frt_renderer* r, uint32_t n, const uint32_t* ids);
int frt_renderer_remove_lights(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode);
int frt_renderer_remove_texture(frt_renderer* r, int kind /*0 colour, 1 data*/, uint32_t layer);
/* For an importer (frt/renderer.py: add_gltf): what frt_scene_add_gltf_materials would add to a scene that has `color_layers` / `data_layers` texture
 * layers, without adding it. materials_out ([materials] of frt_model_counts): the model's materials with their image indices remapped to layer ids;
 * color_images / data_images ([images] each): the image that becomes layer color_layers + k / data_layers + k; counts[2]: how many of each. */
int frt_model_layer_plan(const frt_model* m, uint32_t color_layers, uint32_t data_layers, frt_material* materials_out, uint32_t* color_images, uint32_t* data_images,
                         uint32_t counts[2]);

/* Ray queries against this renderer's scene replica AS IT IS NOW on the device: after every frt_renderer_set_instance_transforms,
 * frt_renderer_set_mesh_vertices and frt_renderer_rebuild_tree so far. Results equal frt_scene_trace_closest / _any over a scene in the same state bit for bit.
 * flags == 0: the pointers are host memory and the call is synchronous (copy up, one kernel, copy down; it returns when `out` is filled).
 * FRT_QUERY_DEVICE: the pointers are 16-byte aligned device memory on the renderer's device; the call only enqueues on the renderer's main stream
 * (frt_renderer_stream(r, 0)) and returns, and the caller orders its reads behind that stream. Allowed at any time, also between the phases of an open
 * frame: a query only reads the scene, and every writer of the scene is on (or fenced into) the main stream. Queries are not counted in frt_stats and
 * touch no frame state. n == 0: FRT_OK, nothing touched. FRT_ERR_INVALID_ARG: null handle, a null pointer with n > 0, n > FRT_QUERY_MAX_RAYS, an
 * unknown flag bit, a misaligned device pointer, and (experiments build) the renderers frt_renderer_rebuild_tree refuses, which do not walk the quad tree. */
#define FRT_QUERY_DEVICE 1u
int frt_renderer_trace_closest(frt_renderer* r, uint32_t n, const frt_ray* rays, frt_ray_hit* out, uint32_t flags);
int frt_renderer_trace_any(frt_renderer* r, uint32_t n, const frt_ray* rays, uint8_t* occluded_out, uint32_t flags);
/* Picking: the closest hit of the primary ray of pixels (xy[2k], xy[2k + 1]) of the renderer's full width x height frame under `cam` (a strip renderer
 * picks in the full frame too: its replica is the whole scene). The ray is made on the device by the code the G-buffer stage uses and traced over its
 * range (0.001, 1000), so a picked hit is the G-buffer's hit: origin + dir * t is FRT_BUF_GPOS.xyz and `material` is its w for that pixel. `cam` is
 * host memory in both forms (copied during the call). A pixel outside the frame: FRT_ERR_INVALID_ARG in the host-pointer form, before anything is
 * enqueued; a miss record under FRT_QUERY_DEVICE. */
int frt_renderer_pick(frt_renderer* r, const frt_camera_uniform* cam, uint32_t n, const uint32_t* xy, frt_ray_hit* out, uint32_t flags);

/* ---- N GPUs behind one call (`ngpus`; section 8e) -----------------------------------------------------------------
 * In the reference one call renders one frame: Renderer::render, src/renderer.rs:349-518, called from State::render, src/state.rs:192-204.
 * frt_multi_renderer is that call for a node with several GPUs: ONE process, `ndev` strip renderers (two-stream schedule), the scene
 * replicated on every device, the frame cut into horizontal strips of equal work, the per-frame halo rows moved by peer copies
 * (hipMemcpyPeerAsync over xGMI) on the right streams, the image gathered when it is read. A Rust `Renderer` over this handle gets N GPUs
 * without knowing about strips. Images are bit-identical to a single frt_renderer's.
 * devices: `ndev` HIP ordinals (NULL = 0 .. ndev-1); an ordinal may repeat (several strips on one GPU: how the path is tested on a 1-GPU box).
 * opts: max_depth, motion_halo_rows (moving camera: rows of previous-frame state exchanged around every strip), queue_capacity and
 * FRT_FLAG_TIMING are honoured; device, stream, rows and arena are set per strip by the library. */
typedef struct frt_multi_renderer frt_multi_renderer;
frt_multi_renderer* frt_multi_renderer_create(const frt_scene* s, uint32_t width, uint32_t height, uint32_t ndev, const int32_t* devices,
                                              const frt_render_opts* opts);                       /* Renderer::new, src/renderer.rs:206 */
void frt_multi_renderer_destroy(frt_multi_renderer* m);
int frt_multi_renderer_render(frt_multi_renderer* m, const frt_camera_uniform* cam);              /* Renderer::render, :349 — asynchronous */
int frt_multi_renderer_sync(frt_multi_renderer* m);
uint32_t frt_multi_renderer_frame_count(const frt_multi_renderer* m);                             /* renderer.frame_count, :198 */
int frt_multi_renderer_reset(frt_multi_renderer* m);                                              /* frame_count = 0, state.rs:152 */
/* A strip whose step fails (a HIP error in the middle of a frame) leaves the other strips with a half-enqueued frame: the handle is then FAILED and
 * every render call returns FRT_ERR_STATE until frt_multi_renderer_clear, which waits for the devices, closes every strip's open frame and puts every
 * strip back into the state right after create (frt_renderer_clear: zeroed targets, frame_count = 0, stats = 0). */
int frt_multi_renderer_clear(frt_multi_renderer* m);
/* PostParams.jitter (renderer.rs:14, :361-379). Only (0, 0) — the shipped reference, camera.rs:202-203 — is accepted when the frame is cut into
 * strips: post's bilinear taps use Repeat addressing and read the opposite image edge (post.wgsl:72-78), which lives on another device. */
int frt_multi_renderer_set_jitter(frt_multi_renderer* m, float jitter_x, float jitter_y);
/* Device-side gather (state.rs:226-278 reads ONE texture per frame): every strip's own rows of `buf`[index] are copied into the full-frame buffer
 * `dst` in the memory of HIP device `device` — peer copies over xGMI on the strips' copy streams, ordered behind the frames enqueued so far, no host
 * staging. `stream` (a hipStream_t of `device`) is ordered behind the copies; stream = NULL: the call returns when the rows have arrived.
 * The next frame's writers of those rows are ordered behind the copies by the library. dst: width * height * bytes-per-pixel of `buf`. */
int frt_multi_renderer_gather(frt_multi_renderer* m, int buf, int index, int32_t device, void* dst, void* stream);
/* out[0] = neighbouring strip pairs on different devices, out[1] = of those, pairs with direct peer access enabled in both directions */
int frt_multi_renderer_peer_access(const frt_multi_renderer* m, uint32_t out[2]);
/* TESTING: the next render call fails on strip `strip` in step `step` (0: T-merge half of the frame, 1: spatial + post half) with FRT_ERR_HIP,
 * as if a HIP call had failed there — how tests reach the failed state above without breaking a device. */
int frt_multi_renderer_inject_failure(frt_multi_renderer* m, uint32_t strip, int step);
/* post_processed_texture, state.rs:226-278: frt_multi_renderer_gather on the first strip's device + ONE device-to-host copy */
int frt_multi_renderer_read_display(frt_multi_renderer* m, uint8_t* rgba8);
int frt_multi_renderer_read_accum(frt_multi_renderer* m, float* rgba32f);
int frt_multi_renderer_read_buffer(frt_multi_renderer* m, int buf, int index, void* out);         /* any target, every strip's own rows */
int frt_multi_renderer_stats(frt_multi_renderer* m, frt_stats* out);                              /* summed over the strips */
int frt_multi_renderer_boundaries(const frt_multi_renderer* m, uint32_t* rows_out);               /* ndev + 1 row indices; returns ndev */
/* frt_renderer_set_instance_transforms on every strip's replica, between frames */
int frt_multi_renderer_set_instance_transforms(frt_multi_renderer* m, uint32_t n, const uint32_t* ids, const float* m_colmajor16);
/* frt_renderer_set_mesh_vertices on every strip's replica, between frames */
int frt_multi_renderer_set_mesh_vertices(frt_multi_renderer* m, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts);
/* ... with flags. FRT_DEFORM_DEVICE is refused (FRT_ERR_INVALID_ARG): the strips' replicas live on different devices. */
int frt_multi_renderer_set_mesh_vertices_ex(frt_multi_renderer* m, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags);
/* frt_renderer_set_mesh_skin and frt_renderer_set_mesh_pose on every strip's replica, between frames. FRT_DEFORM_DEVICE is refused. */
int frt_multi_renderer_set_mesh_skin(frt_multi_renderer* m, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints);
int frt_multi_renderer_set_mesh_skin_ex(frt_multi_renderer* m, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t flags);
int frt_multi_renderer_set_mesh_pose(frt_multi_renderer* m, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags);
/* frt_renderer_set_mesh_morph_targets, frt_renderer_set_mesh_morph_weights and frt_renderer_set_mesh_pose_ex on every strip's replica, between frames.
 * FRT_DEFORM_DEVICE is refused. */
int frt_multi_renderer_set_mesh_morph_targets(frt_multi_renderer* m, uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets);
int frt_multi_renderer_set_mesh_morph_weights(frt_multi_renderer* m, uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags);
int frt_multi_renderer_set_mesh_pose_ex(frt_multi_renderer* m, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* frt_renderer_set_mesh_poses on every strip's replica, between frames. FRT_DEFORM_DEVICE is refused: host arrays only. */
int frt_multi_renderer_set_mesh_poses(frt_multi_renderer* m, uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags);
/* frt_renderer_set_materials, _set_instance_materials, _set_light_emission and _set_texture on every strip's replica, between frames */
int frt_multi_renderer_set_materials(frt_multi_renderer* m, uint32_t n, const uint32_t* ids, const frt_material* materials);
int frt_multi_renderer_set_instance_materials(frt_multi_renderer* m, uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids);
int frt_multi_renderer_set_light_emission(frt_multi_renderer* m, uint32_t light, const float color[3], float intensity);
int frt_multi_renderer_set_texture(frt_multi_renderer* m, int kind, uint32_t layer, const uint8_t* rgba8_1024x1024);
/* frt_renderer_rebuild_tree on every strip's replica, between frames (synchronous) */
int frt_multi_renderer_rebuild_tree(frt_multi_renderer* m);
/* frt_renderer_rebuild_tree_ex on every strip's replica */
int frt_multi_renderer_rebuild_tree_ex(frt_multi_renderer* m, uint32_t mode);
/* frt_renderer_add_instances / _remove_instances on every strip's replica (synchronous). A strip that fails after the first one has changed leaves the
 * handle failed, as a failed render does. */
int frt_multi_renderer_add_instances(frt_multi_renderer* m, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* m_colmajor16, uint32_t rebuild_mode);
int frt_multi_renderer_remove_instances(frt_multi_renderer* m, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode);
/* frt_renderer_add_meshes, _add_materials, _add_texture, _add_lights and _register_quad_light / _sphere_light on every strip's replica. The first strip's
 * refusal leaves every replica as it was; a strip that fails after the first one has changed leaves the handle failed. */
int frt_multi_renderer_add_meshes(frt_multi_renderer* m, uint32_t n, const frt_mesh_data* meshes);
int frt_multi_renderer_add_materials(frt_multi_renderer* m, uint32_t n, const frt_material* materials);
int frt_multi_renderer_add_texture(frt_multi_renderer* m, int kind, const uint8_t* rgba8_1024x1024);
int frt_multi_renderer_add_lights(frt_multi_renderer* m, uint32_t n, const frt_light* lights);
int frt_multi_renderer_register_quad_light(frt_multi_renderer* m, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity, uint32_t rebuild_mode);
int frt_multi_renderer_register_sphere_light(frt_multi_renderer* m, uint32_t mesh_id, const float m_colmajor[16], const float color[3], float intensity, uint32_t rebuild_mode);
/* frt_renderer_remove_materials, _remove_meshes, _remove_lights and _remove_texture on every strip's replica. The first strip's refusal leaves every replica
 * as it was; a strip that fails after the first one has changed leaves the handle failed. */
int frt_multi_renderer_remove_materials(frt_multi_renderer* m, uint32_t n, const uint32_t* ids);
int frt_multi_renderer_remove_meshes(frt_multi_renderer* m, uint32_t n, const uint32_t* ids);
int frt_multi_renderer_remove_lights(frt_multi_renderer* m, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode);
int frt_multi_renderer_remove_texture(frt_multi_renderer* m, int kind, uint32_t layer);
/* The three ray-query calls on the first strip's replica (all replicas are equal). Host-pointer form only: flags must be 0. */
int frt_multi_renderer_trace_closest(frt_multi_renderer* m, uint32_t n, const frt_ray* rays, frt_ray_hit* out, uint32_t flags);
int frt_multi_renderer_trace_any(frt_multi_renderer* m, uint32_t n, const frt_ray* rays, uint8_t* occluded_out, uint32_t flags);
int frt_multi_renderer_pick(frt_multi_renderer* m, const frt_camera_uniform* cam, uint32_t n, const uint32_t* xy, frt_ray_hit* out, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* FRT_H */
