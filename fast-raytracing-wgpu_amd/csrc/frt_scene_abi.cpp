// frt_scene_abi.cpp — the entry points of the C ABI (include/frt.h) that never touch a device: geometry, materials, the scene builder (frt_scene.cpp),
// the camera, and the thread-local message behind frt_last_error, which every other translation unit of the ABI sets through frt::set_error.
#include "frt_renderer_state.hpp"

static thread_local std::string g_err;
int frt::set_error(int code, const std::string& msg) { g_err = msg; return code; }

extern "C" {

const char* frt_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------------------ geometry / materials
int frt_geometry_create(int which, uint32_t subdiv, uint32_t* nverts, uint32_t* nidx, float* pos4, frt_vertex_attr* attrs, uint32_t* idx) {
    Geometry g;
    switch (which) {
    case 0: g = geometry::create_plane(); break;
    case 1: g = geometry::create_cube(); break;
    case 2: if (subdiv > 8) return fail(FRT_ERR_INVALID_ARG, "icosphere subdivisions > 8"); g = geometry::create_sphere(subdiv); break;
    case 3: g = geometry::create_crystal(); break;
    default: return fail(FRT_ERR_INVALID_ARG, "unknown geometry kind");
    }
    if (nverts) *nverts = (uint32_t)g.attributes.size();
    if (nidx) *nidx = (uint32_t)g.indices.size();
    if (pos4) memcpy(pos4, g.positions.data(), g.positions.size() * 4);
    if (attrs) memcpy(attrs, g.attributes.data(), g.attributes.size() * sizeof(frt_vertex_attr));
    if (idx) memcpy(idx, g.indices.data(), g.indices.size() * 4);
    return FRT_OK;
}
void frt_encode_octahedral_normal(const float n[3], float out[2]) { geometry::encode_octahedral_normal(n, out); }
void frt_material_default(const float c[4], frt_material* out) { *out = MaterialBuilder(c[0], c[1], c[2], c[3]); }

// ------------------------------------------------------------------------------------------------ scene
frt_scene* frt_scene_create(void) { return new frt_scene(); }
void frt_scene_destroy(frt_scene* s) { delete s; }

int frt_scene_add_mesh(frt_scene* s, const float* pos4, uint32_t nverts, const frt_vertex_attr* attrs, const uint32_t* idx, uint32_t nidx) {
    if (!s || !pos4 || !attrs || !idx || nverts == 0 || nidx == 0 || nidx % 3 != 0) return fail(FRT_ERR_INVALID_ARG, "add_mesh: bad arguments");
    for (uint32_t i = 0; i < nidx; ++i) if (idx[i] >= nverts) return fail(FRT_ERR_INVALID_ARG, "add_mesh: index out of range");
    Geometry g;
    g.positions.assign(pos4, pos4 + (size_t)nverts * 4);
    g.attributes.assign(attrs, attrs + nverts);
    g.indices.assign(idx, idx + nidx);
    return (int)s->b.add_mesh(g);
}
int frt_scene_add_material(frt_scene* s, const frt_material* m) {
    if (!s || !m) return fail(FRT_ERR_INVALID_ARG, "add_material: null");
    if (s->b.materials.size() >= 0xFFFFu) return fail(FRT_ERR_LIMIT, "more than 65535 materials (custom index packs 16 bits, builder.rs:184)");
    return (int)s->b.add_material(*m);
}
static int check_instance(frt_scene* s, uint32_t mesh_id, uint32_t mat_id, const float* m) {
    if (!s || !m) return fail(FRT_ERR_INVALID_ARG, "instance: null");
    if (mesh_id >= s->b.mesh_infos.size()) return fail(FRT_ERR_INVALID_ARG, "instance: unknown mesh id");
    if (mat_id != 0xFFFFFFFFu && mat_id >= s->b.materials.size()) return fail(FRT_ERR_INVALID_ARG, "instance: unknown material id");
    return FRT_OK;
}
int frt_scene_add_instance(frt_scene* s, uint32_t mesh_id, uint32_t mat_id, const float m[16]) {
    int rc = check_instance(s, mesh_id, mat_id, m);
    if (rc) return rc;
    Mat4 t; memcpy(t.m, m, 64);
    s->b.add_instance(mesh_id, mat_id, t);
    return FRT_OK;
}
int frt_scene_add_light(frt_scene* s, const frt_light* l) {
    if (!s || !l) return fail(FRT_ERR_INVALID_ARG, "add_light: null");
    return (int)s->b.add_light(*l);
}
int frt_scene_register_quad_light(frt_scene* s, uint32_t mesh_id, const float m[16], const float color[3], float intensity) {
    int rc = check_instance(s, mesh_id, 0xFFFFFFFFu, m);
    if (rc) return rc;
    Mat4 t; memcpy(t.m, m, 64);
    s->b.register_quad_light(mesh_id, t, color, intensity);
    return FRT_OK;
}
int frt_scene_register_sphere_light(frt_scene* s, uint32_t mesh_id, const float m[16], const float color[3], float intensity) {
    int rc = check_instance(s, mesh_id, 0xFFFFFFFFu, m);
    if (rc) return rc;
    Mat4 t; memcpy(t.m, m, 64);
    s->b.register_sphere_light(mesh_id, t, color, intensity);
    return FRT_OK;
}
int frt_scene_add_texture(frt_scene* s, int kind, const uint8_t* rgba8) {
    if (!s || !rgba8 || (kind != 0 && kind != 1)) return fail(FRT_ERR_INVALID_ARG, "add_texture: bad arguments");
    auto& v = kind == 0 ? s->b.color_textures : s->b.data_textures;
    if (v.size() >= 0xFFFFu) return fail(FRT_ERR_LIMIT, "too many texture layers");
    return (int)(kind == 0 ? s->b.add_color_texture(rgba8) : s->b.add_data_texture(rgba8));
}
int frt_scene_build(frt_scene* s) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "build: null");
    s->b.build();
    if (!s->b.built) return fail(FRT_ERR_LIMIT, "build: " + s->b.error);
    return FRT_OK;
}
int frt_scene_set_instance_transforms(frt_scene* s, uint32_t n, const uint32_t* ids, const float* m_colmajor16) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: null");
    const int rc = s->b.set_instance_transforms(n, ids, m_colmajor16);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_vertices_ex(frt_scene* s, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: null");
    const int rc = s->b.set_mesh_vertices(mesh_id, pos4, attrs, nverts, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_vertices(frt_scene* s, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts) {
    return frt_scene_set_mesh_vertices_ex(s, mesh_id, pos4, attrs, nverts, 0u);
}
int frt_scene_set_mesh_skin(frt_scene* s, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints) {
    return frt_scene_set_mesh_skin_ex(s, mesh_id, joints4, weights4, nverts, njoints, 0u);
}
int frt_scene_set_mesh_skin_ex(frt_scene* s, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_skin: null");
    const int rc = s->b.set_mesh_skin(mesh_id, joints4, weights4, nverts, njoints, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_pose(frt_scene* s, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_pose: null");
    const int rc = s->b.set_mesh_pose(mesh_id, joint_mats, njoints, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_morph_targets(frt_scene* s, uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_morph_targets: null");
    const int rc = s->b.set_mesh_morph_targets(mesh_id, deltas3, nverts, ntargets);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_morph_weights(frt_scene* s, uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_morph_weights: null");
    const int rc = s->b.set_mesh_morph_weights(mesh_id, weights, ntargets, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_pose_ex(frt_scene* s, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_pose: null");
    const int rc = s->b.set_mesh_pose_ex(mesh_id, joint_mats, njoints, morph_weights, ntargets, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_mesh_poses(frt_scene* s, uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_mesh_poses: null");
    const int rc = s->b.set_mesh_poses(n, mesh_ids, joint_mats, njoints, morph_weights, ntargets, flags);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_materials(frt_scene* s, uint32_t n, const uint32_t* ids, const frt_material* materials) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_materials: null");
    const int rc = s->b.set_materials(n, ids, materials);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_instance_materials(frt_scene* s, uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_instance_materials: null");
    const int rc = s->b.set_instance_materials(n, instance_ids, material_ids);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_light_emission(frt_scene* s, uint32_t light, const float color[3], float intensity) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_light_emission: null");
    const int rc = s->b.set_light_emission(light, color, intensity);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_set_texture(frt_scene* s, int kind, uint32_t layer, const uint8_t* rgba8) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "set_texture: null");
    const int rc = s->b.set_texture(kind, layer, rgba8);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_add_instances(frt_scene* s, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* m_colmajor16) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "add_instances: null");
    const int rc = s->b.add_instances(n, mesh_ids, mat_ids, m_colmajor16);
    return rc < 0 ? fail(rc, s->b.error) : rc;
}
int frt_scene_remove_instances(frt_scene* s, uint32_t n, const uint32_t* ids) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "remove_instances: null");
    const int rc = s->b.remove_instances(n, ids);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_remove_materials(frt_scene* s, uint32_t n, const uint32_t* ids) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "remove_materials: null");
    const int rc = s->b.remove_materials(n, ids);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_remove_meshes(frt_scene* s, uint32_t n, const uint32_t* ids) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "remove_meshes: null");
    const int rc = s->b.remove_meshes(n, ids);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_remove_lights(frt_scene* s, uint32_t n, const uint32_t* ids) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "remove_lights: null");
    const int rc = s->b.remove_lights(n, ids);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
int frt_scene_remove_texture(frt_scene* s, int kind, uint32_t layer) {
    if (!s) return fail(FRT_ERR_INVALID_ARG, "remove_texture: null");
    const int rc = s->b.remove_texture(kind, layer);
    return rc ? fail(rc, s->b.error) : FRT_OK;
}
frt_scene* frt_scene_create_cornell_box(void) {
    frt_scene* s = new frt_scene();
    scenes::create_cornell_box(s->b);
    if (!s->b.built) { g_err = s->b.error; delete s; return nullptr; }
    return s;
}
frt_scene* frt_scene_create_restir_scene(void) {
    frt_scene* s = new frt_scene();
    scenes::create_restir_scene(s->b);
    if (!s->b.built) { g_err = s->b.error; delete s; return nullptr; }
    return s;
}
int frt_scene_counts(const frt_scene* s, uint32_t c[8]) {
    if (!s || !c) return fail(FRT_ERR_INVALID_ARG, "counts: null");
    const SceneBuilder& b = s->b;
    c[0] = (uint32_t)b.tris.size(); c[1] = (uint32_t)b.instances.size(); c[2] = (uint32_t)b.materials.size(); c[3] = (uint32_t)b.lights.size();
    c[4] = (uint32_t)b.mesh_infos.size(); c[5] = (uint32_t)b.attributes.size(); c[6] = (uint32_t)b.indices.size(); c[7] = (uint32_t)b.bvh2.size();
    return FRT_OK;
}
int frt_scene_get(const frt_scene* s, int which, void* out) {
    if (!s || !out) return fail(FRT_ERR_INVALID_ARG, "get: null");
    const SceneBuilder& b = s->b;
    switch (which) {
    case 0: memcpy(out, b.tris.data(), b.tris.size() * sizeof(TriRec)); break;
    case 1: memcpy(out, b.tri_instance.data(), b.tri_instance.size() * 4); break;
    case 2: memcpy(out, b.materials.data(), b.materials.size() * 64); break;
    case 3: memcpy(out, b.lights.data(), b.lights.size() * 64); break;
    case 4: memcpy(out, b.attributes.data(), b.attributes.size() * 32); break;
    case 5: memcpy(out, b.indices.data(), b.indices.size() * 4); break;
    case 6: memcpy(out, b.mesh_infos.data(), b.mesh_infos.size() * 16); break;
    case 7: {
        uint8_t* p = (uint8_t*)out;
        for (const InstanceRec& in : b.instances) {
            const uint32_t h[5] = {in.mesh_id, in.mat_id, in.first_tri, in.tri_count, in.flip};
            memcpy(p, h, 20); memcpy(p + 20, in.m, 64); memcpy(p + 84, in.w2o, 36); p += 120;
        }
    } break;
    case 8: memcpy(out, b.bvh2.data(), b.bvh2.size() * sizeof(frt_bvh2_node)); break;
    case 9: memcpy(out, b.bvh2_tri_index.data(), b.bvh2_tri_index.size() * 4); break;
    case 10: memcpy(out, b.quad_nodes.data(), b.quad_nodes.size() * sizeof(QuadNode)); break;
    case 11: b.ensure_wide8(); memcpy(out, b.wide8.words.data(), b.wide8.words.size() * 4); break;
    case 12: b.ensure_wide8(); memcpy(out, b.tri_slots8.data(), b.tri_slots8.size() * sizeof(TriSlot)); break;
    case 13: memcpy(out, b.tri_slots.data(), b.tri_slots.size() * sizeof(TriSlot)); break;
    case 14: b.ensure_wide8(); memcpy(out, b.wide8.child_boxes.data(), b.wide8.child_boxes.size() * 4); break;
    case 15: memcpy(out, b.pair_nodes.data(), b.pair_nodes.size() * sizeof(PairNode)); break;
    case 16: memcpy(out, b.instances_dev.data(), b.instances_dev.size() * sizeof(InstanceDev)); break;
    case 17: memcpy(out, b.shade_tris.data(), b.shade_tris.size() * sizeof(ShadeTri)); break;
    default: return fail(FRT_ERR_INVALID_ARG, "get: unknown selector");
    }
    return FRT_OK;
}
int frt_scene_bvh_stats(const frt_scene* s, uint32_t st[4]) {
    if (!s || !st) return fail(FRT_ERR_INVALID_ARG, "bvh_stats: null");
    st[0] = s->b.bvh_depth; st[1] = s->b.bvh_leaves; st[2] = s->b.bvh_max_leaf; st[3] = (uint32_t)s->b.pair_nodes.size();
    return FRT_OK;
}
int frt_scene_tree_stats(const frt_scene* s, uint32_t st[8]) {
    if (!s || !st) return fail(FRT_ERR_INVALID_ARG, "tree_stats: null");
    const SceneBuilder& b = s->b;
    b.ensure_wide8();
    st[0] = (uint32_t)b.quad_nodes.size(); st[1] = b.quad_stack_need;
    st[2] = b.wide8.ok ? (uint32_t)(b.wide8.words.size() / kWide8Words) : 0u; st[3] = b.wide8.stack_need; st[4] = b.wide8.depth; st[5] = b.wide8.children;
    st[6] = (uint32_t)b.tri_slots8.size(); st[7] = b.quad_fold;
    return FRT_OK;
}
void frt_camera_default(float aspect, uint32_t frame_count, uint32_t num_lights, frt_camera_uniform* out) {
    camera_default(aspect, frame_count, num_lights, out);
}
int frt_camera_build_uniform(const float position[3], float yaw, float pitch, const float* prev_view_proj, float aspect, uint32_t frame_count,
                             uint32_t num_lights, const float jitter[2], frt_camera_uniform* out, float* unjittered_view_proj) {
    if (!position || !out || !(aspect > 0.0f)) return fail(FRT_ERR_INVALID_ARG, "camera_build_uniform: bad arguments");
    camera_build_uniform(position, yaw, pitch, prev_view_proj, aspect, frame_count, num_lights, jitter ? jitter[0] : 0.0f, jitter ? jitter[1] : 0.0f, out, unjittered_view_proj);
    return FRT_OK;
}
void frt_camera_halton_jitter(uint32_t index, uint32_t width, uint32_t height, float scale, float out[2]) { camera_halton_jitter(index, width, height, scale, out); }

} // extern "C"
