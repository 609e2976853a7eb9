// frt_scene_edit.hip — what edits or reads a renderer's scene replica between frames (include/frt.h): moving instances,
// deforming meshes, the material, light and texture edits (§13), the tree rebuild, adding and removing instances (§14), new meshes, materials, texture
// layers and lights (§15), removing meshes, materials, layers and lights (§16), the ray queries,
// frt_renderer_read_scene and the tree statistics.
// Host code only: the kernels are in frt_refit.hip, frt_deform.hip, frt_material_edit.hip, frt_instance_edit.hip, frt_mesh_edit.hip, frt_scene_remove.hip, frt_rebuild.hip, frt_ploc.hip and frt_query.hip.
#include "frt_renderer_state.hpp"
#include <algorithm>
#include <cstddef>

// Level ranges of a breadth-first tree whose node i has `kids(i, out)` inner children: boundaries of the levels, or empty if the numbering is not
// breadth-first (then the renderer cannot refit).
template <class Kids>
static std::vector<uint32_t> level_ranges(size_t n, Kids kids) {
    std::vector<uint32_t> level(n, 0u), bounds(1, 0u);
    for (size_t i = 0; i < n; ++i) {
        uint32_t c[4]; const int k = kids(i, c);
        for (int j = 0; j < k; ++j) { if (c[j] <= i || c[j] >= n) return {}; level[c[j]] = level[i] + 1u; }
    }
    for (size_t i = 1; i < n; ++i) {
        if (level[i] < level[i - 1]) return {};
        if (level[i] != level[i - 1]) bounds.push_back((uint32_t)i);
    }
    bounds.push_back((uint32_t)n);
    return bounds;
}
int frt::upload_refit_data(frt_renderer* r, const SceneBuilder& b) {
    RefitState& f = r->rf;
    std::vector<float> pos;
    f.pos_offset.clear(); f.index_offset.clear(); f.vert_count.clear(); f.attr_offset.clear(); f.mesh_tris.clear();
    for (size_t m = 0; m < b.mesh_positions.size(); ++m) {
        f.pos_offset.push_back((uint32_t)(pos.size() / 4));
        f.index_offset.push_back(b.mesh_infos[m].index_offset);
        f.vert_count.push_back((uint32_t)(b.mesh_positions[m].size() / 4));
        f.attr_offset.push_back(b.mesh_infos[m].vertex_offset);
        f.mesh_tris.push_back(b.mesh_index_counts[m] / 3u);
        pos.insert(pos.end(), b.mesh_positions[m].begin(), b.mesh_positions[m].end());
    }
    int rc;
    if ((rc = upload(r, pos, &f.d_pos))) return rc;
    if ((rc = upload(r, b.tri_slot_of, &f.d_slot_of))) return rc;
    std::vector<uint32_t> word(4, 0u);
    if ((rc = upload(r, word, &f.d_ext))) return rc;
    f.device_bytes = pos.size() * 4 + b.tri_slot_of.size() * 4 + 16;
    f.inst = b.instances;
    f.lights = b.lights;
    f.color_layers = (uint32_t)b.color_textures.size(); f.data_layers = (uint32_t)b.data_textures.size();
    f.pair_levels = level_ranges(b.pair_nodes.size(), [&](size_t i, uint32_t* c) {
        int k = 0;
        for (int j = 0; j < 2; ++j) { uint32_t ref; memcpy(&ref, &b.pair_nodes[i].q[12 + j], 4); if (!(ref & kLeafFlag)) c[k++] = ref; }
        return k;
    });
    f.quad_levels = level_ranges(b.quad_nodes.size(), [&](size_t i, uint32_t* c) {
        int k = 0;
        for (int j = 0; j < 4; ++j) { uint32_t ref; memcpy(&ref, &b.quad_nodes[i].q[24 + j], 4); if (!(ref & kLeafFlag)) c[k++] = ref; }
        return k;
    });
    f.ok = !f.pair_levels.empty() && !f.quad_levels.empty();
    return FRT_OK;
}

// ------------------------------------------------------------------------------------------------ staging
// The ray queries never synchronised their stream before they replaced their device block (a host-pointer query is synchronous: nothing of an earlier
// one is in flight); here they do, as the two edit calls always did: one wait on an idle stream, and only at a call that grows the block.
int Staging::reserve(size_t h_bytes, size_t d_bytes, hipStream_t stream) {
    if (pending) { HIP_TRY(hipEventSynchronize(ev)); pending = false; }
    if (h_cap < h_bytes) {
        if (h) { HIP_TRY(hipHostFree(h)); h = nullptr; h_cap = 0; }
        HIP_TRY(hipHostMalloc((void**)&h, h_bytes));
        h_cap = h_bytes;
    }
    if (d_cap < d_bytes) {
        HIP_TRY(hipStreamSynchronize(stream));
        if (d) { HIP_TRY(hipFree(d)); d = nullptr; d_cap = 0; }
        HIP_TRY(hipMalloc((void**)&d, d_bytes));
        d_cap = d_bytes;
    }
    return FRT_OK;
}
int Staging::mark(hipStream_t stream) {
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, stream));
    pending = true;
    return FRT_OK;
}
void Staging::release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (ev) (void)hipEventDestroy(ev);
    *this = Staging();
}

// ------------------------------------------------------------------------------------------------ entry checks, stream order
#if FRT_EXPERIMENTS
// lib/libfrt_exp.so only: do this renderer's kernels walk the product's quad tree? That is the tree a refit, a rebuild and a query work on; the 8-wide tree,
// the quantized pair nodes of the resident kernels and the pair tree of the compacting, wavefront, stream and refill kernels are not kept up with it.
static bool walks_quad_tree(const frt_renderer* r) {
    return !(r->walk == kWalkWide || r->walk == kWalkWideLds || r->x.resident || (r->flags & FRT_FLAG_COMPACTION) || r->x.wavefront || r->x.stream_mode || r->x.refill);
}
#endif
// What a call `what` refuses before it looks at its own arguments, in this order: a null handle, then the `parts` it asks for.
enum { kNotFailed = 1, kBetweenFrames = 2, kRefit = 4, kQuadTree = 8, kEditChecks = kNotFailed | kBetweenFrames | kQuadTree,
       kLookChecks = kNotFailed | kBetweenFrames };      // (the edits of §13 involve no tree: every renderer takes them)
static int check_entry(const frt_renderer* r, const std::string& what, unsigned parts) {
    if (!r) return fail(FRT_ERR_INVALID_ARG, what + ": null");
    if ((parts & kNotFailed) && r->failed) return fail(FRT_ERR_STATE, what + ": an earlier frame failed in the middle of its stages; call frt_renderer_clear");
    if ((parts & kBetweenFrames) && r->frame_open) return fail(FRT_ERR_STATE, what + ": a frame is open (call it between frames)");
    if ((parts & kRefit) && !r->rf.ok) return fail(FRT_ERR_STATE, what + ": the scene's trees are not numbered breadth-first");
#if FRT_EXPERIMENTS
    if ((parts & kQuadTree) && !walks_quad_tree(r)) return fail(FRT_ERR_INVALID_ARG, what + ": this renderer's kernels do not walk the quad tree, the only tree this call keeps up or reads");
#endif
    return FRT_OK;
}

// The stream order of a call that writes the scene replica (`drop`: and changes its geometry), on the main stream.
// Ordering: every kernel that reads the scene was enqueued by a finished frame (no frame may be open). Those on the main stream precede the update
// on it; the edge streams' spatial launches are behind the main stream's wait for ev_edge (end of every spatial stage); the ahead stream's work
// (a speculated next frame) is fenced, and a speculation — traced under the old geometry — is dropped as if its camera had not matched. The next
// frame's first kernel is enqueued behind the update on the main stream, or (a new speculation) on the ahead stream behind T-merge's event.
// The fence is unconditional (tail_pending is set first): whatever the ahead stream holds, the main stream waits for it.
static int order_behind_frames(frt_renderer* r, bool drop) {
    if (drop) { const int rc = drop_speculation(r); if (rc) return rc; }
    if (r->ahead) { r->tail_pending = true; return fence_ahead(r); }
    return FRT_OK;
}

extern "C" {

// ------------------------------------------------------------------------------------------------ moving instances
// Ordering: order_behind_frames, the speculation dropped.
// Both trees level by level, deepest first: launch k refits the k-th deepest level of each (after a rebuild the pair tree has no levels left).
static int refit_levels(frt_renderer* r) {
    const RefitState& f = r->rf;
    const size_t lp = f.pair_levels.size() - 1, lq = f.quad_levels.size() - 1;
    for (size_t k = 0; k < std::max(lp, lq); ++k) {
        uint32_t p0 = 0, p1 = 0, q0 = 0, q1 = 0;
        if (k < lp) { p0 = f.pair_levels[lp - 1 - k]; p1 = f.pair_levels[lp - k]; }
        if (k < lq) { q0 = f.quad_levels[lq - 1 - k]; q1 = f.quad_levels[lq - k]; }
        HIP_TRY(launch_refit_level(r->sv, f.d_ext, p0, p1, q0, q1, r->stream));
    }
    return FRT_OK;
}
static int set_instance_transforms_impl(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* mats) {
    RefitState& f = r->rf;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    if (n == 0) return FRT_OK;
    // the records, in the order given (an id given twice: the later record wins, as on the host)
    std::vector<MovedInstance> rec;
    std::vector<int> last(f.inst.size(), -1);
    for (uint32_t k = 0; k < n; ++k) last[ids[k]] = (int)k;
    uint32_t work = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (last[ids[k]] != (int)k) continue;
        InstanceRec& in = f.inst[ids[k]];
        const float* m = mats + 16 * (size_t)k;
        memcpy(in.m, m, sizeof(in.m));
        MovedInstance mi;
        memset(&mi, 0, sizeof(mi));
        mi.id = ids[k]; mi.first_tri = in.first_tri; mi.tri_count = in.tri_count;
        mi.index_offset = f.index_offset[in.mesh_id]; mi.pos_offset = f.pos_offset[in.mesh_id];
        mi.work_begin = work; work += in.tri_count;
        for (int c = 0; c < 4; ++c) for (int a = 0; a < 3; ++a) mi.m[3 * c + a] = m[4 * c + a];
        InstanceDev d;
        memset(&d, 0, sizeof(d));
        d.mesh_id = in.mesh_id; d.mat_id = in.mat_id; d.first_tri = in.first_tri;
        instance_inverse(m, d.w2o, d.flip);
        memcpy(&mi.dev, &d, sizeof(d));
        mi.light = 0xFFFFFFFFu;
        if (in.light >= 0 && (size_t)in.light < f.lights.size()) {
            Mat4 t; memcpy(t.m, m, sizeof(t.m));
            const frt_light l = in.light_kind == 0 ? quad_light_record(t, f.lights[(size_t)in.light].emission) : sphere_light_record(t, f.lights[(size_t)in.light].emission);
            mi.light = (uint32_t)in.light;
            memcpy(&mi.light_rec, &l, sizeof(l));
        }
        rec.push_back(mi);
    }
    // staging: pinned, reused once the previous copy out of it has completed
    const size_t rec_bytes = rec.size() * sizeof(MovedInstance);
    if ((rc = f.rec.reserve(rec_bytes, rec_bytes, r->stream))) return rc;
    memcpy(f.rec.h, rec.data(), rec_bytes);
    HIP_TRY(hipMemcpyAsync(f.rec.d, f.rec.h, rec_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = f.rec.mark(r->stream))) return rc;
    RefitArgs a{reinterpret_cast<const MovedInstance*>(f.rec.d), (uint32_t)rec.size(), work, f.d_pos, f.d_slot_of, const_cast<unsigned int*>(f.d_ext)};
    HIP_TRY(launch_instance_transform(r->sv, a, r->stream));
    return refit_levels(r);
}
int frt_renderer_set_instance_transforms(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* m_colmajor16) {
    if (const int rc = check_entry(r, "set_instance_transforms", kEditChecks | kRefit)) return rc;
    const std::string bad = check_instance_transforms(n, ids, m_colmajor16, r->rf.inst.size());
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: " + bad);
    const int rc = set_instance_transforms_impl(r, n, ids, m_colmajor16);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// ------------------------------------------------------------------------------------------------ deforming meshes ("Deforming meshes")
// Ordering as the instance update's. One pinned block holds what a call uploads: [positions | attributes | instance records | decoded normals];
// the first two are copied into the replica (the object-space positions the instance update reads, SceneView::attributes), the last two into a
// device buffer of this call's own. The block is reused once the previous call's copies out of it have completed (Staging::ev); the device buffer is
// reused in stream order and replaced, after a wait for the stream, only when it has to grow.
static int set_mesh_vertices_impl(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts) {
    RefitState& f = r->rf;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    std::vector<DeformInstance> rec;
    uint32_t work = 0;
    for (size_t i = 0; i < f.inst.size(); ++i) {      // in instance order
        const InstanceRec& in = f.inst[i];
        if (in.mesh_id != mesh_id) continue;
        DeformInstance d;
        d.id = (uint32_t)i; d.first_tri = in.first_tri; d.tri_count = in.tri_count; d.work_begin = work; work += in.tri_count;
        for (int c = 0; c < 4; ++c) for (int a = 0; a < 3; ++a) d.m[3 * c + a] = in.m[4 * c + a];
        rec.push_back(d);
    }
    const size_t pos_bytes = (size_t)nverts * 16, attr_bytes = attrs ? (size_t)nverts * sizeof(frt_vertex_attr) : 0;
    const size_t rec_bytes = rec.size() * sizeof(DeformInstance), nrm_bytes = attrs ? (size_t)nverts * 16 : 0;
    const size_t up_bytes = rec_bytes + nrm_bytes, all_bytes = pos_bytes + attr_bytes + up_bytes;
    if ((rc = f.def.reserve(all_bytes, up_bytes, r->stream))) return rc;
    uint8_t* h_pos = f.def.h; uint8_t* h_attr = h_pos + pos_bytes; uint8_t* h_up = h_attr + attr_bytes;
    memcpy(h_pos, pos4, pos_bytes);
    if (attrs) {
        memcpy(h_attr, attrs, attr_bytes);
        float* nrm = reinterpret_cast<float*>(h_up + rec_bytes);
        for (uint32_t v = 0; v < nverts; ++v) { decoded_vertex_normal(attrs[v], nrm + 4 * (size_t)v); nrm[4 * (size_t)v + 3] = 0.0f; }
    }
    if (rec_bytes) memcpy(h_up, rec.data(), rec_bytes);
    HIP_TRY(hipMemcpyAsync(const_cast<float4*>(f.d_pos) + f.pos_offset[mesh_id], h_pos, pos_bytes, hipMemcpyHostToDevice, r->stream));
    if (attrs) HIP_TRY(hipMemcpyAsync(const_cast<VertexAttrView*>(r->sv.attributes) + f.attr_offset[mesh_id], h_attr, attr_bytes, hipMemcpyHostToDevice, r->stream));
    if (up_bytes) HIP_TRY(hipMemcpyAsync(f.def.d, h_up, up_bytes, hipMemcpyHostToDevice, r->stream));
    if (attrs && r->ie.d_normals)      // (what a later frt_renderer_add_instances of this mesh reads, §14)
        HIP_TRY(hipMemcpyAsync(const_cast<float4*>(r->ie.d_normals) + f.attr_offset[mesh_id], h_up + rec_bytes, nrm_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = f.def.mark(r->stream))) return rc;
    if (work == 0) return FRT_OK;      // no instance of the mesh: no triangle changes
    DeformArgs a{reinterpret_cast<const DeformInstance*>(f.def.d), (uint32_t)rec.size(), work, f.index_offset[mesh_id], f.pos_offset[mesh_id], f.attr_offset[mesh_id],
                 f.d_pos, attrs ? reinterpret_cast<const float4*>(f.def.d + rec_bytes) : nullptr, f.d_slot_of};
    HIP_TRY(launch_mesh_deform(r->sv, a, r->stream));
    HIP_TRY(launch_scene_extent(r->sv, const_cast<unsigned int*>(f.d_ext), r->stream));
    return refit_levels(r);
}
int frt_renderer_set_mesh_vertices(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts) {
    if (const int rc = check_entry(r, "set_mesh_vertices", kEditChecks | kRefit)) return rc;
    if (mesh_id >= r->rf.vert_count.size())
        return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: mesh id " + std::to_string(mesh_id) + " out of range (" + std::to_string(r->rf.vert_count.size()) + " meshes)");
    const std::string bad = check_mesh_vertices(pos4, attrs, nverts, r->rf.vert_count[mesh_id]);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: " + bad);
    const int rc = set_mesh_vertices_impl(r, mesh_id, pos4, attrs, nverts);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// ------------------------------------------------------------------------------------------------ materials, lights, textures
// Ordering as the instance update's (order_behind_frames, the speculation dropped: its G-buffer and T-trace have read the materials). All four calls
// stage through r->look: what a call uploads is written into the pinned block and copied from there, on the main stream, into the replica's tables
// (or, for the instance records of set_instance_materials, into the device block its one kernel reads). The pinned block is reused once the
// previous call's copies out of it have completed (Staging::ev).
static int set_materials_impl(frt_renderer* r, uint32_t n, const uint32_t* ids, const frt_material* mats) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    // ascending ids, of an id given twice its last value: no two copies overlap, and a run of consecutive ids is one copy
    std::vector<std::pair<uint32_t, uint32_t>> e(n);
    for (uint32_t k = 0; k < n; ++k) e[k] = {ids[k], k};
    std::sort(e.begin(), e.end());
    size_t m = 0;
    for (size_t k = 0; k < e.size(); ++k) if (k + 1 == e.size() || e[k + 1].first != e[k].first) e[m++] = e[k];
    e.resize(m);
    if ((rc = r->look.reserve(m * sizeof(frt_material), 0, r->stream))) return rc;
    for (size_t k = 0; k < m; ++k) memcpy(r->look.h + k * sizeof(frt_material), mats + e[k].second, sizeof(frt_material));
    for (size_t k = 0; k < m;) {
        size_t run = 1;
        while (k + run < m && e[k + run].first == e[k].first + (uint32_t)run) ++run;
        HIP_TRY(hipMemcpyAsync(const_cast<MaterialView*>(r->sv.materials) + e[k].first, r->look.h + k * sizeof(frt_material), run * sizeof(frt_material), hipMemcpyHostToDevice, r->stream));
        k += run;
    }
    return r->look.mark(r->stream);
}
int frt_renderer_set_materials(frt_renderer* r, uint32_t n, const uint32_t* ids, const frt_material* materials) {
    if (const int rc = check_entry(r, "set_materials", kLookChecks)) return rc;
    const std::string bad = check_set_materials(n, ids, materials, r->sv.num_materials, r->rf.color_layers, r->rf.data_layers, r->sv.num_lights);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_materials: " + bad);
    if (n == 0) return FRT_OK;
    const int rc = set_materials_impl(r, n, ids, materials);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int set_instance_materials_impl(frt_renderer* r, uint32_t n, const uint32_t* iids, const uint32_t* mids) {
    RefitState& f = r->rf;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    // one record per distinct instance (an id given twice: its last value), so that no two threads of the kernel store the same word
    std::vector<MaterialEditInstance> rec;
    std::vector<int> last(f.inst.size(), -1);
    for (uint32_t k = 0; k < n; ++k) last[iids[k]] = (int)k;
    uint32_t work = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (last[iids[k]] != (int)k) continue;
        InstanceRec& in = f.inst[iids[k]];
        in.mat_id = mids[k];      // (the record a later set_instance_transforms re-creates carries it)
        rec.push_back(MaterialEditInstance{in.first_tri, work, iids[k], mids[k]});
        work += in.tri_count;
    }
    const size_t rec_bytes = rec.size() * sizeof(MaterialEditInstance);
    if ((rc = r->look.reserve(rec_bytes, rec_bytes, r->stream))) return rc;
    memcpy(r->look.h, rec.data(), rec_bytes);
    HIP_TRY(hipMemcpyAsync(r->look.d, r->look.h, rec_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = r->look.mark(r->stream))) return rc;
    const MaterialEditArgs a{reinterpret_cast<const MaterialEditInstance*>(r->look.d), (uint32_t)rec.size(), work, (uint32_t)f.inst.size()};
    HIP_TRY(launch_instance_materials(r->sv, a, r->stream));
    return FRT_OK;
}
int frt_renderer_set_instance_materials(frt_renderer* r, uint32_t n, const uint32_t* instance_ids, const uint32_t* material_ids) {
    if (const int rc = check_entry(r, "set_instance_materials", kLookChecks)) return rc;
    const std::string bad = check_set_instance_materials(n, instance_ids, material_ids, r->rf.inst, r->sv.num_materials);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_instance_materials: " + bad);
    if (n == 0) return FRT_OK;
    const int rc = set_instance_materials_impl(r, n, instance_ids, material_ids);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int set_light_emission_impl(frt_renderer* r, uint32_t light, const float color[3], float intensity) {
    RefitState& f = r->rf;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    float up[8] = {color[0], color[1], color[2], intensity, 0.0f, 0.0f, 0.0f, 0.0f};      // [emission | emissive_factor]
    light_emissive_factor(color, intensity, up + 4);
    memcpy(f.lights[light].emission, up, 16);      // the mirror a later set_instance_transforms re-creates a moved light's record from
    if ((rc = r->look.reserve(sizeof(up), 0, r->stream))) return rc;
    memcpy(r->look.h, up, sizeof(up));
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(const_cast<LightView*>(r->sv.lights) + light) + offsetof(LightView, emission), r->look.h, 16, hipMemcpyHostToDevice, r->stream));
    const int i = light_instance(f.inst, light);
    if (i >= 0 && f.inst[(size_t)i].mat_id < r->sv.num_materials)
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(const_cast<MaterialView*>(r->sv.materials) + f.inst[(size_t)i].mat_id) + offsetof(MaterialView, emissive_factor), r->look.h + 16, 12, hipMemcpyHostToDevice, r->stream));
    return r->look.mark(r->stream);
}
int frt_renderer_set_light_emission(frt_renderer* r, uint32_t light, const float color[3], float intensity) {
    if (const int rc = check_entry(r, "set_light_emission", kLookChecks)) return rc;
    if (!color) return fail(FRT_ERR_INVALID_ARG, "set_light_emission: null colour");
    if (light >= r->sv.num_lights) return fail(FRT_ERR_INVALID_ARG, "set_light_emission: light " + std::to_string(light) + " out of range (" + std::to_string(r->sv.num_lights) + " lights)");
    const int rc = set_light_emission_impl(r, light, color, intensity);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int set_texture_impl(frt_renderer* r, int kind, uint32_t layer, const uint8_t* rgba8) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    if ((rc = r->look.reserve(kTextureLayerBytes, 0, r->stream))) return rc;
    memcpy(r->look.h, rgba8, kTextureLayerBytes);
    uint8_t* dst = const_cast<uint8_t*>(kind == 0 ? r->sv.color_tex : r->sv.data_tex) + (size_t)layer * kTextureLayerBytes;
    HIP_TRY(hipMemcpyAsync(dst, r->look.h, kTextureLayerBytes, hipMemcpyHostToDevice, r->stream));
    return r->look.mark(r->stream);
}
int frt_renderer_set_texture(frt_renderer* r, int kind, uint32_t layer, const uint8_t* rgba8) {
    if (const int rc = check_entry(r, "set_texture", kLookChecks)) return rc;
    const std::string bad = check_set_texture(kind, layer, rgba8, r->rf.color_layers, r->rf.data_layers);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_texture: " + bad);
    const int rc = set_texture_impl(r, kind, layer, rgba8);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// ------------------------------------------------------------------------------------------------ tree rebuild ("Rebuild")
// Ordering: as the instance update, the ahead stream is fenced into the main stream (the edge streams already are, behind ev_edge). A speculated
// frame that ran ahead on the old tree is kept: both trees give the same hits. The call waits for the main stream, so when it returns no kernel
// reads the buffers that left the replica; they stay allocated and are what the next rebuild builds into.
// Scene allocations that may be replaced while the renderer lives (they are freed with the scene replica otherwise).
static int scene_alloc(frt_renderer* r, size_t bytes, void** out) {
    HIP_TRY(hipMalloc(out, std::max<size_t>(bytes, 16)));
    r->scene_allocs.push_back(*out);
    return FRT_OK;
}
static void scene_free(frt_renderer* r, const void* p) {
    if (!p) return;
    auto it = std::find(r->scene_allocs.begin(), r->scene_allocs.end(), const_cast<void*>(p));
    if (it != r->scene_allocs.end()) r->scene_allocs.erase(it);
    (void)hipFree(const_cast<void*>(p));
}
// Triangles the replica's triangle-sized buffers have room for: their count until an instance edit gave them a capacity.
static uint32_t tri_capacity(const frt_renderer* r) { return r->ie.cap_tris ? r->ie.cap_tris : r->sv.num_tris; }

// The buffers a rebuild builds into, with room for a tree over tri_capacity() triangles: the scratch, the spare triangle slots and id -> slot table, and
// the quad-node buffer that is not in use. Each is (re)allocated only when it is too small; none of them is part of the replica, and no kernel of an
// earlier call still uses them (every rebuild waits for its stream).
static int rebuild_prepare(frt_renderer* r, uint32_t num_tris, uint32_t mode, RebuildTarget& target) {
    RebuildState& b = r->rbt;
    const uint32_t cap = std::max(tri_capacity(r), num_tris);
    int rc;
    if (b.cap_tris < cap) {
        const size_t had = b.scratch.bytes + b.scratch.ploc.bytes;
        HIP_TRY(rebuild_reserve(b.scratch, cap));
        b.device_bytes += b.scratch.bytes + b.scratch.ploc.bytes; b.device_bytes -= had;
        scene_free(r, b.tris); scene_free(r, b.slot_of);
        b.device_bytes -= (uint64_t)b.cap_tris * (sizeof(TriSlot) + sizeof(uint32_t));
        b.tris = nullptr; b.slot_of = nullptr; b.cap_tris = 0;
        if ((rc = scene_alloc(r, (size_t)cap * sizeof(TriSlot), (void**)&b.tris))) return rc;
        if ((rc = scene_alloc(r, (size_t)cap * sizeof(uint32_t), (void**)&b.slot_of))) return rc;
        b.cap_tris = cap;
        b.device_bytes += (uint64_t)cap * (sizeof(TriSlot) + sizeof(uint32_t));
    }
    if (mode == FRT_REBUILD_SAH && num_tris > 2u) {      // the refined mode's own scratch, at its first call (and after a growth) only
        const size_t had = b.scratch.ploc.bytes;
        HIP_TRY(ploc_reserve(b.scratch, cap));
        b.device_bytes += b.scratch.ploc.bytes - had;
    }
    const int t = r->sv.nodes4 == b.nodes[0] ? 1 : 0;
    const uint32_t need = rebuild_max_nodes(cap);
    if (b.nodes_cap[t] < need) {
        scene_free(r, b.nodes[t]);
        b.device_bytes -= (uint64_t)b.nodes_cap[t] * sizeof(QuadNode);
        b.nodes[t] = nullptr; b.nodes_cap[t] = 0;
        if ((rc = scene_alloc(r, (size_t)need * sizeof(QuadNode), (void**)&b.nodes[t]))) return rc;
        b.nodes_cap[t] = need;
        b.device_bytes += (uint64_t)need * sizeof(QuadNode);
    }
    target = RebuildTarget{b.tris, b.nodes[t], b.slot_of};
    return FRT_OK;
}
// The tree of `src` (its tris and num_tris; `src_slot_of` its id -> slot table) into the buffers of rebuild_prepare, and the checks every caller makes before
// anything of the replica changes. Waits for the main stream.
static int rebuild_into(frt_renderer* r, const SceneView& src, const uint32_t* src_slot_of, uint32_t mode, const char* what, RebuildTarget& target, RebuildResult& res) {
    RebuildState& b = r->rbt;
    if (const int rc = rebuild_prepare(r, src.num_tris, mode, target)) return rc;
    HIP_TRY(rebuild_tree(b.scratch, src, src_slot_of, target, const_cast<unsigned int*>(r->rf.d_ext), r->stream, res, mode));
    b.last[0] = mode; b.last[1] = res.iterations; b.last[2] = res.fell_back; b.last[3] = (uint32_t)((b.scratch.ploc.bytes + 1023u) >> 10);
    if (res.num_nodes == 0) return fail(FRT_ERR_LIMIT, std::string(what) + ": the tree could not be numbered (nothing changed)");
    // the kernels have no overflow check: the bound is hard, and it is checked before anything of the replica changes
    if (res.stack_need > (uint32_t)kStackDepth - 1u)
        return fail(FRT_ERR_LIMIT, std::string(what) + ": the new tree needs " + std::to_string(res.stack_need) + " traversal-stack entries, " + std::to_string(kStackDepth - 1) + " is the limit (nothing changed)");
    return FRT_OK;
}
// The finished tree enters the replica; the buffers that leave it are what the next rebuild builds into.
static void rebuild_swap(frt_renderer* r, const RebuildTarget& target, const RebuildResult& res) {
    RebuildState& b = r->rbt;
    SceneView& sv = r->sv;
    b.tris = const_cast<float4*>(sv.tris); b.slot_of = const_cast<uint32_t*>(r->rf.d_slot_of);
    sv.tris = target.tris; r->rf.d_slot_of = target.slot_of;
    sv.nodes4 = target.nodes; sv.num_nodes4 = res.num_nodes;
    r->rf.quad_levels = res.levels;
    r->rf.pair_levels.assign(1, 0u);       // later refits skip the pair levels
    r->rf.ok = true;
    r->wg_rows = res.stack_need + 1u;
    r->vote = res.num_nodes >= kVoteMinQuadNodes;
    b.done = true; b.origin = res.origin;
}
static int rebuild_tree_impl(frt_renderer* r, uint32_t mode) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, false);
    if (rc) return rc;
    RebuildTarget target;
    RebuildResult res;
    if ((rc = rebuild_into(r, r->sv, r->rf.d_slot_of, mode, "rebuild_tree", target, res))) return rc;
    rebuild_swap(r, target, res);
    return FRT_OK;
}
int frt_renderer_rebuild_tree(frt_renderer* r) { return frt_renderer_rebuild_tree_ex(r, FRT_REBUILD_MORTON); }
int frt_renderer_rebuild_tree_ex(frt_renderer* r, uint32_t mode) {
    if (const int rc = check_entry(r, "rebuild_tree", kEditChecks)) return rc;
    if (mode != FRT_REBUILD_MORTON && mode != FRT_REBUILD_SAH) return fail(FRT_ERR_INVALID_ARG, "rebuild_tree: unknown mode (FRT_REBUILD_MORTON, FRT_REBUILD_SAH)");
    const int rc = rebuild_tree_impl(r, mode);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}
// ------------------------------------------------------------------------------------------------ adding and removing instances
// Ordering: as the instance update's (order_behind_frames, the speculation dropped: it was traced on the old geometry). The kernels of
// frt_instance_edit.hip write buffers that are not part of the replica (InstanceEditState); the scene-extent pass and the rebuild follow them on the
// main stream and read only those; the rebuild waits for the stream, and only then — the tree is known to fit the traversal stack — do the new
// triangles, shading records, instance records, id -> slot table and tree enter the replica in one step, with the host bookkeeping (RefitState::inst).
// A call that is refused or fails before that step leaves the replica as it was (the extent word is made again from the replica's triangles).

// Room for `need_tris` triangles and `need_inst` instances in every buffer sized by them: the replica's (triangle slots, id -> slot table, shading
// records, instance records: new allocation + device-to-device copy of what is in use) and the edit's own; the rebuild's buffers follow in
// rebuild_prepare. Capacities double (at least), are never shrunk, and nothing happens while they suffice.
// (`elem`: bytes per element; `live` / `own` point at the caller's pointer of whatever type)
static int grow_live(frt_renderer* r, const void* live_ptr, size_t elem, size_t used, size_t cap) {
    const void** live = static_cast<const void**>(const_cast<void*>(live_ptr));
    void* d = nullptr;
    if (const int rc = scene_alloc(r, cap * elem, &d)) return rc;
    if (used) HIP_TRY(hipMemcpy(d, *live, used * elem, hipMemcpyDeviceToDevice));
    scene_free(r, *live);
    *live = d;
    return FRT_OK;
}
static int regrow_own(frt_renderer* r, void* own_ptr, size_t elem, size_t cap) {
    void** own = static_cast<void**>(own_ptr);
    scene_free(r, *own); *own = nullptr;
    return scene_alloc(r, cap * elem, own);
}
static int reserve_edit(frt_renderer* r, uint32_t need_tris, uint32_t need_inst) {
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    const uint32_t have_tris = tri_capacity(r), have_inst = e.cap_inst ? e.cap_inst : (uint32_t)r->rf.inst.size();
    const bool first = e.tris == nullptr, more_tris = need_tris > have_tris, more_inst = need_inst > have_inst;
    if (!first && !more_tris && !more_inst) return FRT_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));      // (the ahead stream is fenced into it: no kernel reads what is replaced below)
    int rc;
    if (first || more_tris) {
        const uint32_t cap = more_tris ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need_tris, 2ull * have_tris), kMaxSceneTris) : have_tris;
        if (more_tris) {
            if ((rc = grow_live(r, &sv.tris, sizeof(TriSlot), sv.num_tris, cap))) return rc;
            if ((rc = grow_live(r, &sv.shade_tris, sizeof(ShadeTri), sv.num_tris, cap))) return rc;
            if ((rc = grow_live(r, &r->rf.d_slot_of, sizeof(uint32_t), sv.num_tris, cap))) return rc;
        }
        if ((rc = regrow_own(r, &e.tris, sizeof(TriSlot), cap))) return rc;
        if ((rc = regrow_own(r, &e.shade_tris, sizeof(ShadeTri), cap))) return rc;
        if ((rc = regrow_own(r, &e.slot_of, sizeof(uint32_t), cap))) return rc;
        e.cap_tris = cap;
    }
    if (first || more_inst) {
        const uint32_t cap = more_inst ? std::max(need_inst, 2u * have_inst) : have_inst;
        if (more_inst && (rc = grow_live(r, &sv.instances, sizeof(InstanceView), r->rf.inst.size(), cap))) return rc;
        if ((rc = regrow_own(r, &e.instances, sizeof(InstanceView), cap))) return rc;
        e.cap_inst = cap;
    }
    if (more_tris || more_inst) ++e.growths;
    return FRT_OK;
}
// The decoded normal of every vertex of the replica, made once, at the first call that adds an instance: the attributes come back from the device (a
// deformation may have replaced them) and are decoded by the function build_gpu_layout uses.
static int ensure_normals(frt_renderer* r) {
    if (r->ie.d_normals) return FRT_OK;
    const RefitState& f = r->rf;
    const size_t nverts = f.attr_offset.empty() ? 0 : (size_t)f.attr_offset.back() + f.vert_count.back();
    std::vector<frt_vertex_attr> attrs(nverts);
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (nverts) HIP_TRY(hipMemcpy(attrs.data(), r->sv.attributes, nverts * sizeof(frt_vertex_attr), hipMemcpyDeviceToHost));
    std::vector<float> nrm(4 * nverts, 0.0f);
    for (size_t v = 0; v < nverts; ++v) decoded_vertex_normal(attrs[v], &nrm[4 * v]);
    void* d = nullptr;      // (with room for the vertex pool's capacity, which a growth or a removal has set apart from its count)
    if (const int rc = scene_alloc(r, std::max<size_t>(nverts, r->me.cap[kPoolVerts]) * sizeof(float4), &d)) return rc;
    if (nverts) HIP_TRY(hipMemcpy(d, nrm.data(), nrm.size() * sizeof(float), hipMemcpyHostToDevice));
    r->ie.d_normals = static_cast<const float4*>(d);
    return FRT_OK;
}
// What both calls end with: the extent and the tree of the triangles the edit wrote, then everything enters the replica together.
static int commit_instance_edit(frt_renderer* r, uint32_t num_tris, std::vector<InstanceRec>& inst, uint32_t mode, const char* what) {
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    unsigned int* ext = const_cast<unsigned int*>(r->rf.d_ext);
    SceneView nv = sv;
    nv.tris = e.tris; nv.shade_tris = e.shade_tris; nv.instances = e.instances; nv.num_tris = num_tris;
    HIP_TRY(launch_scene_extent(nv, ext, r->stream));
    RebuildTarget target;
    RebuildResult res;
    const int rc = rebuild_into(r, nv, e.slot_of, mode, what, target, res);
    if (rc) {
        if (rc != FRT_ERR_HIP) {      // refused: the extent word of the replica's own triangles again (fail()'s message is kept)
            HIP_TRY(launch_scene_extent(sv, ext, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
        }
        return rc;
    }
    rebuild_swap(r, target, res);      // (what left the replica there are the spare slots and table of the next rebuild)
    { float4* was = const_cast<float4*>(sv.shade_tris); sv.shade_tris = e.shade_tris; e.shade_tris = was; }
    { InstanceView* was = const_cast<InstanceView*>(sv.instances); sv.instances = e.instances; e.instances = was; }
    sv.num_tris = num_tris;
    r->rf.inst.swap(inst);
    return FRT_OK;
}

// (`light` >= 0, register_*_light of §15: the first new instance carries the link to that light, of kind `light_kind`)
static int add_instances_impl(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats, uint32_t mode, int32_t light = -1, uint32_t light_kind = 0) {
    RefitState& f = r->rf;
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old_tris = sv.num_tris, old_inst = (uint32_t)f.inst.size();
    std::vector<InstanceRec> inst = f.inst;
    std::vector<AppendInstance> rec(n);
    uint32_t work = 0;
    for (uint32_t k = 0; k < n; ++k) {      // in argument order: the next instance ids, the next flattened triangle ids
        const float* m = mats + 16 * (size_t)k;
        InstanceRec in{};
        in.mesh_id = mesh_ids[k]; in.mat_id = mat_ids[k]; in.first_tri = old_tris + work; in.tri_count = f.mesh_tris[mesh_ids[k]];
        memcpy(in.m, m, sizeof(in.m));
        instance_inverse(m, in.w2o, in.flip);
        AppendInstance& a = rec[k];
        memset(&a, 0, sizeof(a));
        a.id = old_inst + k; a.first_tri = in.first_tri; a.tri_count = in.tri_count; a.work_begin = work;
        a.index_offset = f.index_offset[in.mesh_id]; a.pos_offset = f.pos_offset[in.mesh_id]; a.attr_offset = f.attr_offset[in.mesh_id];
        for (int c = 0; c < 4; ++c) for (int x = 0; x < 3; ++x) a.m[3 * c + x] = m[4 * c + x];
        a.dev.mesh_id = in.mesh_id; a.dev.mat_id = in.mat_id; a.dev.first_tri = in.first_tri; a.dev.flip = in.flip;
        memcpy(a.dev.w2o, in.w2o, sizeof(in.w2o));
        work += in.tri_count;
        if (k == 0 && light >= 0) { in.light = light; in.light_kind = light_kind; }
        inst.push_back(in);
    }
    const uint32_t num_tris = old_tris + work, num_inst = old_inst + n;
    if ((rc = reserve_edit(r, num_tris, num_inst))) return rc;
    if ((rc = ensure_normals(r))) return rc;
    const size_t rec_bytes = rec.size() * sizeof(AppendInstance);
    if ((rc = e.rec.reserve(rec_bytes, rec_bytes, r->stream))) return rc;
    memcpy(e.rec.h, rec.data(), rec_bytes);
    HIP_TRY(hipMemcpyAsync(e.rec.d, e.rec.h, rec_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = e.rec.mark(r->stream))) return rc;
    // what stays: the old slots where they are (and their table), the old shading and instance records
    HIP_TRY(hipMemcpyAsync(e.tris, sv.tris, (size_t)old_tris * sizeof(TriSlot), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(e.slot_of, f.d_slot_of, (size_t)old_tris * sizeof(uint32_t), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(e.shade_tris, sv.shade_tris, (size_t)old_tris * sizeof(ShadeTri), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(e.instances, sv.instances, (size_t)old_inst * sizeof(InstanceView), hipMemcpyDeviceToDevice, r->stream));
    const AppendArgs a{reinterpret_cast<const AppendInstance*>(e.rec.d), n, work, f.d_pos, e.d_normals, num_tris, num_inst, InstanceEditTarget{e.tris, e.slot_of, e.shade_tris, e.instances}};
    HIP_TRY(launch_instances_append(sv, a, r->stream));
    if ((rc = commit_instance_edit(r, num_tris, inst, mode, "add_instances"))) return rc;
    return (int)old_inst;
}

static int remove_instances_impl(frt_renderer* r, const std::vector<uint32_t>& gone, uint32_t mode) {
    RefitState& f = r->rf;
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old_tris = sv.num_tris, old_inst = (uint32_t)f.inst.size();
    std::vector<RemovedRange> rng;
    std::vector<InstanceRec> inst;
    uint32_t tris_gone = 0;
    size_t g = 0;
    for (uint32_t i = 0; i < old_inst; ++i) {
        if (g < gone.size() && gone[g] == i) {
            const uint32_t before = tris_gone;
            tris_gone += f.inst[i].tri_count;
            rng.push_back(RemovedRange{f.inst[i].first_tri - before, tris_gone, i - (uint32_t)g, 0u});
            ++g;
            continue;
        }
        InstanceRec in = f.inst[i];
        in.first_tri -= tris_gone;
        inst.push_back(in);
    }
    const uint32_t num_tris = old_tris - tris_gone, num_inst = (uint32_t)inst.size();
    if (num_tris == 0) return fail(FRT_ERR_INVALID_ARG, "remove_instances: no triangle would be left (nothing changed)");
    if ((rc = reserve_edit(r, num_tris, num_inst))) return rc;
    const size_t rec_bytes = rng.size() * sizeof(RemovedRange);
    if ((rc = e.rec.reserve(rec_bytes, rec_bytes, r->stream))) return rc;
    memcpy(e.rec.h, rng.data(), rec_bytes);
    HIP_TRY(hipMemcpyAsync(e.rec.d, e.rec.h, rec_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = e.rec.mark(r->stream))) return rc;
    const RemoveArgs a{reinterpret_cast<const RemovedRange*>(e.rec.d), (uint32_t)rng.size(), f.d_slot_of, old_tris, old_inst, num_tris, num_inst,
                       InstanceEditTarget{e.tris, e.slot_of, e.shade_tris, e.instances}};
    HIP_TRY(launch_instances_remove(sv, a, r->stream));
    return commit_instance_edit(r, num_tris, inst, mode, "remove_instances");
}

static int check_rebuild_mode(const char* what, uint32_t mode) {
    if (mode != FRT_REBUILD_MORTON && mode != FRT_REBUILD_SAH) return fail(FRT_ERR_INVALID_ARG, std::string(what) + ": unknown rebuild mode (FRT_REBUILD_MORTON, FRT_REBUILD_SAH)");
    return FRT_OK;
}
int frt_renderer_add_instances(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* m_colmajor16, uint32_t rebuild_mode) {
    if (const int rc = check_entry(r, "add_instances", kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode("add_instances", rebuild_mode)) return rc;
    std::string why;
    if (const int rc = check_add_instances(n, mesh_ids, mat_ids, m_colmajor16, r->rf.mesh_tris, r->sv.num_materials, r->sv.num_tris, why)) return fail(rc, "add_instances: " + why);
    if (n == 0) return (int)r->rf.inst.size();
    const int rc = add_instances_impl(r, n, mesh_ids, mat_ids, m_colmajor16, rebuild_mode);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}
int frt_renderer_remove_instances(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode) {
    if (const int rc = check_entry(r, "remove_instances", kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode("remove_instances", rebuild_mode)) return rc;
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_instances(n, ids, r->rf.inst, gone, why)) return fail(rc, "remove_instances: " + why);
    if (gone.empty()) return FRT_OK;
    const int rc = remove_instances_impl(r, gone, rebuild_mode);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}
int frt_renderer_scene_counts(frt_renderer* r, uint32_t counts[4]) {
    if (!r || !counts) return fail(FRT_ERR_INVALID_ARG, "renderer scene_counts: null");
    counts[0] = r->sv.num_tris; counts[1] = (uint32_t)r->rf.inst.size(); counts[2] = r->sv.num_materials; counts[3] = r->sv.num_lights;
    return FRT_OK;
}

// ------------------------------------------------------------------------------------------------ new meshes, materials, layers, lights
// Ordering: as the edits of §13 (order_behind_frames, the speculation dropped). What a call uploads is written into the pinned block of r->me.up and
// copied from there, on the main stream: materials, lights and texture layers straight into the replica's pools, the vertices and indices of new meshes
// into the device block mesh_append_kernel reads. A pool that is too small grows first (reserve_pools): behind a wait for the stream, by a new
// allocation and a device-to-device copy of what is in use. The host bookkeeping (RefitState) and the counts of the SceneView follow when everything
// is enqueued, so that the edits of §11 - §14 accept the new ids.
static uint32_t pool_verts(const frt_renderer* r) { const RefitState& f = r->rf; return f.attr_offset.empty() ? 0u : f.attr_offset.back() + f.vert_count.back(); }
static uint32_t pool_indices(const frt_renderer* r) { const RefitState& f = r->rf; return f.index_offset.empty() ? 0u : f.index_offset.back() + 3u * f.mesh_tris.back(); }
static uint32_t pool_count(const frt_renderer* r, int pool) {
    switch (pool) {
    case kPoolVerts: return pool_verts(r);
    case kPoolIndices: return pool_indices(r);
    case kPoolMeshes: return (uint32_t)r->rf.mesh_tris.size();
    case kPoolMaterials: return r->sv.num_materials;
    case kPoolLights: return r->sv.num_lights;
    case kPoolColor: return r->rf.color_layers;
    default: return r->rf.data_layers;
    }
}
// grow_live for a pool: an allocation that fails is a limit, not a broken device (nothing has changed then).
static int grow_pool(frt_renderer* r, const void* live_ptr, size_t elem, size_t used, size_t cap) {
    const void** live = static_cast<const void**>(const_cast<void*>(live_ptr));
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(cap * elem, 16)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FRT_ERR_LIMIT, "no device memory for " + std::to_string(cap * elem) + " bytes (nothing changed)");
    }
    r->scene_allocs.push_back(d);
    if (used) HIP_TRY(hipMemcpy(d, *live, used * elem, hipMemcpyDeviceToDevice));
    scene_free(r, *live);
    *live = d;
    return FRT_OK;
}
// Room for `need[pool]` elements in every pool (0: the pool is not asked about). A pool's capacity is its count until it first grows.
static int reserve_pools(frt_renderer* r, const uint32_t need[kPoolCount]) {
    MeshEditState& e = r->me;
    SceneView& sv = r->sv;
    bool synced = false, grew = false;
    for (int p = 0; p < kPoolCount; ++p) {
        const uint32_t used = pool_count(r, p), have = e.cap[p] ? e.cap[p] : used;
        if (need[p] <= have) continue;
        if (!synced) { HIP_TRY(hipStreamSynchronize(r->stream)); synced = true; }      // (the ahead stream is fenced into it: no kernel reads what is replaced below)
        const uint32_t cap = p == kPoolColor || p == kPoolData ? grown_layer_capacity(have, need[p])
                           : grown_capacity(have, need[p], p == kPoolMaterials ? kMaxMaterials : kMaxPoolElems);
        int rc = FRT_OK;
        switch (p) {
        case kPoolVerts:
            if ((rc = grow_pool(r, &r->rf.d_pos, sizeof(float4), used, cap))) return rc;
            if ((rc = grow_pool(r, &sv.attributes, sizeof(VertexAttrView), used, cap))) return rc;
            if ((rc = grow_pool(r, &r->ie.d_normals, sizeof(float4), used, cap))) return rc;
            break;
        case kPoolIndices: rc = grow_pool(r, &sv.indices, sizeof(uint32_t), used, cap); break;
        case kPoolMeshes: rc = grow_pool(r, &sv.mesh_infos, sizeof(MeshInfoView), used, cap); break;
        case kPoolMaterials: rc = grow_pool(r, &sv.materials, sizeof(MaterialView), used, cap); break;
        case kPoolLights: rc = grow_pool(r, &sv.lights, sizeof(LightView), used, cap); break;
        case kPoolColor: rc = grow_pool(r, &sv.color_tex, kTextureLayerBytes, used, cap); break;
        default: rc = grow_pool(r, &sv.data_tex, kTextureLayerBytes, used, cap); break;
        }
        if (rc) return rc;
        e.cap[p] = cap;
        grew = true;
    }
    if (grew) ++e.growths;
    return FRT_OK;
}
// `bytes` from `src` through the pinned block at `h_off` to `dst`, on the main stream (the caller has reserved the block and marks it afterwards).
static int staged_copy(frt_renderer* r, size_t h_off, const void* src, void* dst, size_t bytes) {
    memcpy(r->me.up.h + h_off, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, r->me.up.h + h_off, bytes, hipMemcpyHostToDevice, r->stream));
    return FRT_OK;
}

static int add_meshes_impl(frt_renderer* r, uint32_t n, const frt_mesh_data* meshes) {
    RefitState& f = r->rf;
    MeshEditState& e = r->me;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old_meshes = (uint32_t)f.mesh_tris.size(), old_verts = pool_verts(r), old_indices = pool_indices(r);
    std::vector<MeshAppend> rec;
    uint32_t nv = 0, ni = 0;
    pack_mesh_appends(n, meshes, old_verts, old_indices, rec, nv, ni);
    if ((rc = ensure_normals(r))) return rc;      // (at the replica's present size; the pool of the vertices grows with the others below)
    uint32_t need[kPoolCount] = {};
    need[kPoolVerts] = old_verts + nv; need[kPoolIndices] = old_indices + ni; need[kPoolMeshes] = old_meshes + n;
    if ((rc = reserve_pools(r, need))) return rc;
    // one block: [records | positions | attributes | indices], each part 16-byte aligned (32 n, 16 nv and 32 nv bytes in front of the indices)
    const size_t rec_bytes = (size_t)n * sizeof(MeshAppend), pos_bytes = (size_t)nv * 16, attr_bytes = (size_t)nv * sizeof(frt_vertex_attr), idx_bytes = (size_t)ni * 4;
    const size_t pos_at = rec_bytes, attr_at = pos_at + pos_bytes, idx_at = attr_at + attr_bytes, all_bytes = idx_at + idx_bytes;
    if ((rc = e.up.reserve(all_bytes, all_bytes, r->stream))) return rc;
    memcpy(e.up.h, rec.data(), rec_bytes);
    for (uint32_t k = 0; k < n; ++k) {
        memcpy(e.up.h + pos_at + (size_t)rec[k].vert_begin * 16, meshes[k].pos4, (size_t)meshes[k].nverts * 16);
        memcpy(e.up.h + attr_at + (size_t)rec[k].vert_begin * sizeof(frt_vertex_attr), meshes[k].attrs, (size_t)meshes[k].nverts * sizeof(frt_vertex_attr));
        memcpy(e.up.h + idx_at + (size_t)rec[k].index_begin * 4, meshes[k].idx, (size_t)meshes[k].nidx * 4);
    }
    HIP_TRY(hipMemcpyAsync(e.up.d, e.up.h, all_bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = e.up.mark(r->stream))) return rc;
    MeshAppendArgs a{};
    a.rec = reinterpret_cast<const MeshAppend*>(e.up.d); a.nrec = n; a.nverts = nv; a.nidx = ni;
    a.pos = reinterpret_cast<const float4*>(e.up.d + pos_at); a.attrs = reinterpret_cast<const float4*>(e.up.d + attr_at); a.idx = reinterpret_cast<const uint32_t*>(e.up.d + idx_at);
    a.out_pos = const_cast<float4*>(f.d_pos); a.out_attrs = reinterpret_cast<float4*>(const_cast<VertexAttrView*>(r->sv.attributes));
    a.out_normals = const_cast<float4*>(r->ie.d_normals); a.out_idx = const_cast<uint32_t*>(r->sv.indices); a.out_infos = const_cast<MeshInfoView*>(r->sv.mesh_infos);
    a.mesh_base = old_meshes;
    a.cap_verts = e.cap[kPoolVerts] ? e.cap[kPoolVerts] : old_verts; a.cap_indices = e.cap[kPoolIndices] ? e.cap[kPoolIndices] : old_indices;
    a.cap_meshes = e.cap[kPoolMeshes] ? e.cap[kPoolMeshes] : old_meshes;
    HIP_TRY(launch_mesh_append(a, r->stream));
    for (uint32_t k = 0; k < n; ++k) {
        f.pos_offset.push_back(rec[k].vert_base); f.attr_offset.push_back(rec[k].vert_base); f.index_offset.push_back(rec[k].index_base);
        f.vert_count.push_back(rec[k].nverts); f.mesh_tris.push_back(rec[k].nidx / 3u);
    }
    return (int)old_meshes;
}
int frt_renderer_add_meshes(frt_renderer* r, uint32_t n, const frt_mesh_data* meshes) {
    if (const int rc = check_entry(r, "add_meshes", kLookChecks)) return rc;
    const RefitState& f = r->rf;
    const uint64_t pos_verts = f.pos_offset.empty() ? 0u : (uint64_t)f.pos_offset.back() + f.vert_count.back();
    if (pos_verts != pool_verts(r)) return fail(FRT_ERR_STATE, "add_meshes: the replica's positions and attributes are not numbered alike");
    std::string why;
    if (const int rc = check_add_meshes(n, meshes, pool_verts(r), pool_indices(r), why)) return fail(rc, "add_meshes: " + why);
    if (n == 0) return (int)f.mesh_tris.size();
    uint64_t work = 0;
    for (uint32_t k = 0; k < n; ++k) work += (uint64_t)meshes[k].nverts + meshes[k].nidx;
    if (work > 0xFFFFFF00ull || (uint64_t)f.mesh_tris.size() + n > 0x7FFFFFFFull) return fail(FRT_ERR_LIMIT, "add_meshes: too many vertices and indices, or meshes, in one call");
    const int rc = add_meshes_impl(r, n, meshes);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int add_materials_impl(frt_renderer* r, uint32_t n, const frt_material* mats) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old = r->sv.num_materials;
    uint32_t need[kPoolCount] = {};
    need[kPoolMaterials] = old + n;
    if ((rc = reserve_pools(r, need))) return rc;
    const size_t bytes = (size_t)n * sizeof(frt_material);
    if ((rc = r->me.up.reserve(bytes, 0, r->stream))) return rc;
    if ((rc = staged_copy(r, 0, mats, const_cast<MaterialView*>(r->sv.materials) + old, bytes))) return rc;
    if ((rc = r->me.up.mark(r->stream))) return rc;
    r->sv.num_materials = old + n;
    return (int)old;
}
int frt_renderer_add_materials(frt_renderer* r, uint32_t n, const frt_material* materials) {
    if (const int rc = check_entry(r, "add_materials", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_materials(n, materials, r->sv.num_materials, r->rf.color_layers, r->rf.data_layers, r->sv.num_lights, why)) return fail(rc, "add_materials: " + why);
    if (n == 0) return (int)r->sv.num_materials;
    const int rc = add_materials_impl(r, n, materials);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int add_texture_impl(frt_renderer* r, int kind, const uint8_t* rgba8) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    uint32_t& layers = kind == 0 ? r->rf.color_layers : r->rf.data_layers;
    uint32_t need[kPoolCount] = {};
    need[kind == 0 ? kPoolColor : kPoolData] = layers + 1u;
    if ((rc = reserve_pools(r, need))) return rc;
    if ((rc = r->me.up.reserve(kTextureLayerBytes, 0, r->stream))) return rc;
    uint8_t* dst = const_cast<uint8_t*>(kind == 0 ? r->sv.color_tex : r->sv.data_tex) + (size_t)layers * kTextureLayerBytes;
    if ((rc = staged_copy(r, 0, rgba8, dst, kTextureLayerBytes))) return rc;
    if ((rc = r->me.up.mark(r->stream))) return rc;
    return (int)layers++;
}
int frt_renderer_add_texture(frt_renderer* r, int kind, const uint8_t* rgba8) {
    if (const int rc = check_entry(r, "add_texture", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_texture(kind, rgba8, r->rf.color_layers, r->rf.data_layers, why)) return fail(rc, "add_texture: " + why);
    const int rc = add_texture_impl(r, kind, rgba8);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int add_lights_impl(frt_renderer* r, uint32_t n, const frt_light* lights) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old = r->sv.num_lights;
    uint32_t need[kPoolCount] = {};
    need[kPoolLights] = old + n;
    if ((rc = reserve_pools(r, need))) return rc;
    const size_t bytes = (size_t)n * sizeof(frt_light);
    if ((rc = r->me.up.reserve(bytes, 0, r->stream))) return rc;
    if ((rc = staged_copy(r, 0, lights, const_cast<LightView*>(r->sv.lights) + old, bytes))) return rc;
    if ((rc = r->me.up.mark(r->stream))) return rc;
    r->rf.lights.insert(r->rf.lights.end(), lights, lights + n);
    r->sv.num_lights = old + n;
    return (int)old;
}
int frt_renderer_add_lights(frt_renderer* r, uint32_t n, const frt_light* lights) {
    if (const int rc = check_entry(r, "add_lights", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_lights(n, lights, why)) return fail(rc, "add_lights: " + why);
    if ((uint64_t)r->sv.num_lights + n > 0x7FFFFFFFull) return fail(FRT_ERR_LIMIT, "add_lights: a material's light_index is a signed 32-bit number");
    if (n == 0) return (int)r->sv.num_lights;
    const int rc = add_lights_impl(r, n, lights);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// register_quad_light / register_sphere_light of the builder (frt_scene.cpp) on the replica: the material and the light record are made by the builder's
// own functions; the pools get their room first (a refusal there changes nothing), then the instance goes through add_instances_impl with the ids the
// material and the light are about to get, and only when its tree is in place do the two records follow and the counts move.
static int register_light_impl(frt_renderer* r, uint32_t mesh_id, const float* m, const frt_material& mat, const frt_light& light, uint32_t kind, uint32_t mode) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t mat_id = r->sv.num_materials, light_id = r->sv.num_lights;
    uint32_t need[kPoolCount] = {};
    need[kPoolMaterials] = mat_id + 1u; need[kPoolLights] = light_id + 1u;
    if ((rc = reserve_pools(r, need))) return rc;
    if ((rc = r->me.up.reserve(sizeof(mat) + sizeof(light), 0, r->stream))) return rc;
    if ((rc = add_instances_impl(r, 1, &mesh_id, &mat_id, m, mode, (int32_t)light_id, kind)) < 0) return rc;
    if ((rc = staged_copy(r, 0, &mat, const_cast<MaterialView*>(r->sv.materials) + mat_id, sizeof(mat)))) return rc;
    if ((rc = staged_copy(r, sizeof(mat), &light, const_cast<LightView*>(r->sv.lights) + light_id, sizeof(light)))) return rc;
    if ((rc = r->me.up.mark(r->stream))) return rc;
    r->rf.lights.push_back(light);
    r->sv.num_materials = mat_id + 1u; r->sv.num_lights = light_id + 1u;
    return (int)light_id;
}
static int register_light(frt_renderer* r, uint32_t mesh_id, const float* m, const float* color, float intensity, uint32_t mode, uint32_t kind, const char* what) {
    if (const int rc = check_entry(r, what, kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode(what, mode)) return rc;
    if (!m || !color) return fail(FRT_ERR_INVALID_ARG, std::string(what) + ": null matrix or colour");
    const uint32_t mat_id = r->sv.num_materials;
    std::string why;
    if (mat_id >= kMaxMaterials) return fail(FRT_ERR_LIMIT, std::string(what) + ": more than 65535 materials");
    if (const int rc = check_add_instances(1, &mesh_id, &mat_id, m, r->rf.mesh_tris, (size_t)mat_id + 1u, r->sv.num_tris, why)) return fail(rc, std::string(what) + ": " + why);
    Mat4 t; memcpy(t.m, m, sizeof(t.m));
    const float em[4] = {color[0], color[1], color[2], intensity};
    const frt_light light = kind == 0 ? quad_light_record(t, em) : sphere_light_record(t, em);
    if (const int rc = check_add_lights(1, &light, why)) return fail(rc, std::string(what) + ": the light this transform, colour and intensity make: " + why);
    const frt_material mat = light_emissive_material(r->sv.num_lights, color, intensity);
    const int rc = register_light_impl(r, mesh_id, m, mat, light, kind, mode);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}
int frt_renderer_register_quad_light(frt_renderer* r, uint32_t mesh_id, const float m[16], const float color[3], float intensity, uint32_t rebuild_mode) {
    return register_light(r, mesh_id, m, color, intensity, rebuild_mode, 0u, "register_quad_light");
}
int frt_renderer_register_sphere_light(frt_renderer* r, uint32_t mesh_id, const float m[16], const float color[3], float intensity, uint32_t rebuild_mode) {
    return register_light(r, mesh_id, m, color, intensity, rebuild_mode, 1u, "register_sphere_light");
}
int frt_renderer_pool_counts(frt_renderer* r, uint32_t counts[6]) {
    if (!r || !counts) return fail(FRT_ERR_INVALID_ARG, "renderer pool_counts: null");
    counts[0] = pool_count(r, kPoolMeshes); counts[1] = pool_verts(r); counts[2] = pool_indices(r);
    counts[3] = r->rf.color_layers; counts[4] = r->rf.data_layers; counts[5] = r->me.growths;
    return FRT_OK;
}

// ------------------------------------------------------------------------------------------------ removing meshes, materials, layers, lights
// Ordering: as the edits of §13 (order_behind_frames, the speculation dropped: it has read the ids that change). The tables of a call (old -> new ids,
// removed spans) are staged through r->rm.tab. A pool that closes up is compacted by a kernel into its spare buffer (RemoveState), which enters the
// replica on the host once every launch of the call is enqueued; the buffer that left is the next removal's spare, and the next kernel that writes it
// is behind this call's readers on the same stream. Surviving records are renumbered in place, one word per thread, and so is gpos.w of every G-buffer
// set the renderer owns. Nothing waits for the device unless a spare has to be (re)allocated, except the two checks that read the material table back.
static uint32_t pool_cap(const frt_renderer* r, int p) { return r->me.cap[p] ? r->me.cap[p] : pool_count(r, p); }
static void pin_capacity(frt_renderer* r, int p) { if (!r->me.cap[p]) r->me.cap[p] = pool_count(r, p); }      // before the count moves: the buffer keeps its room
static int spare_for(frt_renderer* r, int slot, size_t bytes, void** out) {
    RemoveState& s = r->rm;
    if (!s.spare[slot] || s.spare_bytes[slot] < bytes) {
        HIP_TRY(hipStreamSynchronize(r->stream));      // (a kernel of an earlier call may still read what is freed)
        scene_free(r, s.spare[slot]);
        s.spare[slot] = nullptr; s.spare_bytes[slot] = 0;
        if (const int rc = scene_alloc(r, bytes, &s.spare[slot])) return rc;
        s.spare_bytes[slot] = std::max<size_t>(bytes, 16);
    }
    *out = s.spare[slot];
    return FRT_OK;
}
// The replica's buffer `live` and the spare of `slot` trade places (`live_bytes`: what the buffer that leaves has room for).
static void swap_spare(frt_renderer* r, int slot, const void* live_ptr, size_t live_bytes) {
    const void** live = static_cast<const void**>(const_cast<void*>(live_ptr));
    RemoveState& s = r->rm;
    void* was = const_cast<void*>(*live);
    *live = s.spare[slot];
    s.spare[slot] = was; s.spare_bytes[slot] = std::max<size_t>(live_bytes, 16);
}
static int stage_words(frt_renderer* r, const std::vector<uint32_t>& w, const uint32_t** d) {
    const size_t bytes = std::max<size_t>(w.size() * 4, 16);
    Staging& t = r->rm.tab;
    if (const int rc = t.reserve(bytes, bytes, r->stream)) return rc;
    memcpy(t.h, w.data(), w.size() * 4);
    HIP_TRY(hipMemcpyAsync(t.d, t.h, bytes, hipMemcpyHostToDevice, r->stream));
    if (const int rc = t.mark(r->stream)) return rc;
    *d = reinterpret_cast<const uint32_t*>(t.d);
    return FRT_OK;
}
// [map of `count` ids | one span per removed id] for a pool of single records.
static std::vector<uint32_t> id_tables(size_t count, const std::vector<uint32_t>& gone, std::vector<uint32_t>& map) {
    map = removal_map(count, gone);
    std::vector<uint32_t> w = map;
    for (size_t k = 0; k < gone.size(); ++k) { w.push_back(gone[k] - (uint32_t)k); w.push_back((uint32_t)k + 1u); }
    return w;
}
// gpos.w of every G-buffer set this renderer owns, over all its rows.
static int remap_history(frt_renderer* r, const uint32_t* d_map, uint32_t n) {
    for (uint32_t g = 0; g < r->gsets && g < (uint32_t)kGSets; ++g) {
        const int b = B_GPOS0 + (int)g;
        if (is_extra(b) && !r->extras) continue;
        HIP_TRY(launch_remap_history(static_cast<float4*>(r->buf(b)), r->W * r->H, d_map, n, r->stream));
    }
    return FRT_OK;
}
// The material table as it is on the device (the checks of remove_lights and remove_texture read light_index and the texture slots): waits for the device.
static int read_materials(frt_renderer* r, std::vector<frt_material>& out) {
    FRT_DEVICE(r);
    if (const int rc = sync_all(r)) return rc;
    out.resize(r->sv.num_materials);
    if (!out.empty()) HIP_TRY(hipMemcpy(out.data(), r->sv.materials, out.size() * sizeof(frt_material), hipMemcpyDeviceToHost));
    return FRT_OK;
}

// The materials `gone` (checked, not empty) leave the table; instance records, shading records and the per-pixel history follow. The caller has ordered the stream.
static int remove_materials_device(frt_renderer* r, const std::vector<uint32_t>& gone) {
    SceneView& sv = r->sv;
    const uint32_t old = sv.num_materials, left = old - (uint32_t)gone.size();
    std::vector<uint32_t> map;
    const std::vector<uint32_t> words = id_tables(old, gone, map);
    pin_capacity(r, kPoolMaterials);
    const size_t cap_bytes = (size_t)pool_cap(r, kPoolMaterials) * sizeof(MaterialView);
    void* dst = nullptr;
    int rc;
    if ((rc = spare_for(r, kSpareMaterials, cap_bytes, &dst))) return rc;
    const uint32_t* d = nullptr;
    if ((rc = stage_words(r, words, &d))) return rc;
    const RemovedSpan* spans = reinterpret_cast<const RemovedSpan*>(d + old);
    HIP_TRY(launch_compact_vec4(reinterpret_cast<const float4*>(sv.materials), static_cast<float4*>(dst), left, 4u, spans, (uint32_t)gone.size(), r->stream));
    HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<float4*>(sv.shade_tris)), sv.num_tris, 32u, 25u, d, old, r->stream));
    HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<InstanceView*>(sv.instances)), (uint32_t)r->rf.inst.size(), 16u, 1u, d, old, r->stream));
    if ((rc = remap_history(r, d, old))) return rc;
    swap_spare(r, kSpareMaterials, &sv.materials, cap_bytes);
    for (InstanceRec& in : r->rf.inst) if (in.mat_id < old && map[in.mat_id] != kGone) in.mat_id = map[in.mat_id];
    sv.num_materials = left;
    return FRT_OK;
}
// The light records `gone` (checked, not empty) leave the table; light_index of every material and the light link of every instance follow.
static int remove_light_records_device(frt_renderer* r, const std::vector<uint32_t>& gone) {
    SceneView& sv = r->sv;
    const uint32_t old = sv.num_lights, left = old - (uint32_t)gone.size();
    std::vector<uint32_t> map;
    const std::vector<uint32_t> words = id_tables(old, gone, map);
    pin_capacity(r, kPoolLights);
    const size_t cap_bytes = (size_t)pool_cap(r, kPoolLights) * sizeof(LightView);
    void* dst = nullptr;
    int rc;
    if ((rc = spare_for(r, kSpareLights, cap_bytes, &dst))) return rc;
    const uint32_t* d = nullptr;
    if ((rc = stage_words(r, words, &d))) return rc;
    const RemovedSpan* spans = reinterpret_cast<const RemovedSpan*>(d + old);
    HIP_TRY(launch_compact_vec4(reinterpret_cast<const float4*>(sv.lights), static_cast<float4*>(dst), left, 4u, spans, (uint32_t)gone.size(), r->stream));
    HIP_TRY(launch_remap_materials(const_cast<MaterialView*>(sv.materials), sv.num_materials, d, old, kGone, kGone, r->stream));
    swap_spare(r, kSpareLights, &sv.lights, cap_bytes);
    remove_elements(r->rf.lights, gone);
    for (InstanceRec& in : r->rf.inst) if (in.light >= 0 && (uint32_t)in.light < old && map[(size_t)in.light] != kGone) in.light = (int32_t)map[(size_t)in.light];
    sv.num_lights = left;
    return FRT_OK;
}

static int remove_materials_impl(frt_renderer* r, const std::vector<uint32_t>& gone) {
    FRT_DEVICE(r);
    if (const int rc = order_behind_frames(r, true)) return rc;
    return remove_materials_device(r, gone);
}
int frt_renderer_remove_materials(frt_renderer* r, uint32_t n, const uint32_t* ids) {
    if (const int rc = check_entry(r, "remove_materials", kLookChecks)) return rc;
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_materials(n, ids, r->sv.num_materials, r->rf.inst, gone, why)) return fail(rc, "remove_materials: " + why);
    if (gone.empty()) return FRT_OK;
    const int rc = remove_materials_impl(r, gone);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

static int remove_meshes_impl(frt_renderer* r, const std::vector<uint32_t>& gone) {
    RefitState& f = r->rf;
    SceneView& sv = r->sv;
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    const uint32_t old_meshes = (uint32_t)f.mesh_tris.size(), old_verts = pool_verts(r), old_indices = pool_indices(r);
    std::vector<uint32_t> index_count(old_meshes);
    for (uint32_t m = 0; m < old_meshes; ++m) index_count[m] = 3u * f.mesh_tris[m];
    std::vector<RemovedSpan> sm, sve, si;
    pack_mesh_removal(gone, f.attr_offset, f.vert_count, f.index_offset, index_count, sm, sve, si);
    const uint32_t ns = (uint32_t)gone.size(), verts = old_verts - sve.back().through, indices = old_indices - si.back().through, meshes = old_meshes - ns;
    const std::vector<uint32_t> map = removal_map(old_meshes, gone);
    std::vector<uint32_t> words(6u * ns);      // [mesh spans | vertex spans | index spans | old -> new mesh ids]
    memcpy(words.data(), sm.data(), 8u * ns); memcpy(words.data() + 2u * ns, sve.data(), 8u * ns); memcpy(words.data() + 4u * ns, si.data(), 8u * ns);
    words.insert(words.end(), map.begin(), map.end());
    pin_capacity(r, kPoolVerts); pin_capacity(r, kPoolIndices); pin_capacity(r, kPoolMeshes);
    const size_t cv = pool_cap(r, kPoolVerts), ci = pool_cap(r, kPoolIndices), cm = pool_cap(r, kPoolMeshes);
    void *pos = nullptr, *attrs = nullptr, *nrm = nullptr, *idx = nullptr, *infos = nullptr;
    if ((rc = spare_for(r, kSparePos, cv * sizeof(float4), &pos))) return rc;
    if ((rc = spare_for(r, kSpareAttrs, cv * sizeof(VertexAttrView), &attrs))) return rc;
    if (r->ie.d_normals && (rc = spare_for(r, kSpareNormals, cv * sizeof(float4), &nrm))) return rc;
    if ((rc = spare_for(r, kSpareIndices, ci * sizeof(uint32_t), &idx))) return rc;
    if ((rc = spare_for(r, kSpareMeshInfos, cm * sizeof(MeshInfoView), &infos))) return rc;
    const uint32_t* d = nullptr;
    if ((rc = stage_words(r, words, &d))) return rc;
    const RemovedSpan *dm = reinterpret_cast<const RemovedSpan*>(d), *dv = dm + ns, *di = dv + ns;
    HIP_TRY(launch_compact_vec4(f.d_pos, static_cast<float4*>(pos), verts, 1u, dv, ns, r->stream));
    HIP_TRY(launch_compact_vec4(reinterpret_cast<const float4*>(sv.attributes), static_cast<float4*>(attrs), verts, 2u, dv, ns, r->stream));
    if (nrm) HIP_TRY(launch_compact_vec4(r->ie.d_normals, static_cast<float4*>(nrm), verts, 1u, dv, ns, r->stream));
    HIP_TRY(launch_compact_u32(sv.indices, static_cast<uint32_t*>(idx), indices, di, ns, r->stream));
    HIP_TRY(launch_compact_mesh_infos(sv.mesh_infos, static_cast<MeshInfoView*>(infos), meshes, dm, dv, di, ns, r->stream));
    HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<InstanceView*>(sv.instances)), (uint32_t)f.inst.size(), 16u, 0u, d + 6u * ns, old_meshes, r->stream));
    // everything is enqueued: the new pools enter the replica together, with the host bookkeeping
    swap_spare(r, kSparePos, &f.d_pos, cv * sizeof(float4));
    swap_spare(r, kSpareAttrs, &sv.attributes, cv * sizeof(VertexAttrView));
    if (nrm) swap_spare(r, kSpareNormals, &r->ie.d_normals, cv * sizeof(float4));
    swap_spare(r, kSpareIndices, &sv.indices, ci * sizeof(uint32_t));
    swap_spare(r, kSpareMeshInfos, &sv.mesh_infos, cm * sizeof(MeshInfoView));
    std::vector<uint32_t> vo, io, vc, mt;
    uint32_t v = 0, i = 0;
    for (uint32_t m = 0; m < old_meshes; ++m) {      // the offsets a scratch build gives the survivors
        if (map[m] == kGone) continue;
        vo.push_back(v); io.push_back(i); vc.push_back(f.vert_count[m]); mt.push_back(f.mesh_tris[m]);
        v += f.vert_count[m]; i += index_count[m];
    }
    f.pos_offset = vo; f.attr_offset.swap(vo); f.index_offset.swap(io); f.vert_count.swap(vc); f.mesh_tris.swap(mt);
    for (InstanceRec& in : f.inst) in.mesh_id = map[in.mesh_id];
    return FRT_OK;
}
int frt_renderer_remove_meshes(frt_renderer* r, uint32_t n, const uint32_t* ids) {
    if (const int rc = check_entry(r, "remove_meshes", kLookChecks)) return rc;
    const RefitState& f = r->rf;
    if (f.pos_offset != f.attr_offset) return fail(FRT_ERR_STATE, "remove_meshes: the replica's positions and attributes are not numbered alike");
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_meshes(n, ids, f.mesh_tris.size(), f.inst, gone, why)) return fail(rc, "remove_meshes: " + why);
    if (gone.empty()) return FRT_OK;
    if (2ull * pool_verts(r) > 0xFFFFFF00ull || pool_indices(r) > 0xFFFFFF00u) return fail(FRT_ERR_LIMIT, "remove_meshes: too many vertices or indices for one compaction launch");
    const int rc = remove_meshes_impl(r, gone);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// A registered light leaves as the composite register_*_light made: its instance first (remove_instances_impl: the one step that can be refused, by the
// tree; nothing has changed then), then its material, then the record.
static int remove_lights_impl(frt_renderer* r, const LightRemoval& rem, uint32_t mode) {
    FRT_DEVICE(r);
    int rc = order_behind_frames(r, true);
    if (rc) return rc;
    if (!rem.instances.empty() && (rc = remove_instances_impl(r, rem.instances, mode))) return rc;
    if (!rem.materials.empty() && (rc = remove_materials_device(r, rem.materials))) return rc;      // (from here on only a HIP call can fail: the renderer is then failed)
    return remove_light_records_device(r, rem.lights);
}
int frt_renderer_remove_lights(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode) {
    if (const int rc = check_entry(r, "remove_lights", kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode("remove_lights", rebuild_mode)) return rc;
    if (n == 0) return FRT_OK;
    std::vector<frt_material> mats;
    if (const int rc = read_materials(r, mats)) { if (rc == FRT_ERR_HIP) r->failed = true; return rc; }
    LightRemoval rem;
    std::string why;
    if (const int rc = check_remove_lights(n, ids, r->sv.num_lights, mats.data(), mats.size(), r->rf.inst, rem, why)) return fail(rc, "remove_lights: " + why);
    if (rem.lights.empty()) return FRT_OK;
    const int rc = remove_lights_impl(r, rem, rebuild_mode);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// The layers above the removed one move down, one device-to-device copy each in ascending order (source and destination of a copy are different layers;
// a copy's destination is the source of the copy before it, which the stream has finished by then).
static int remove_texture_impl(frt_renderer* r, int kind, uint32_t layer) {
    FRT_DEVICE(r);
    if (const int rc = order_behind_frames(r, true)) return rc;
    pin_capacity(r, kind == 0 ? kPoolColor : kPoolData);
    uint32_t& layers = kind == 0 ? r->rf.color_layers : r->rf.data_layers;
    uint8_t* base = const_cast<uint8_t*>(kind == 0 ? r->sv.color_tex : r->sv.data_tex);
    for (uint32_t l = layer; l + 1u < layers; ++l)
        HIP_TRY(hipMemcpyAsync(base + (size_t)l * kTextureLayerBytes, base + (size_t)(l + 1u) * kTextureLayerBytes, kTextureLayerBytes, hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(launch_remap_materials(const_cast<MaterialView*>(r->sv.materials), r->sv.num_materials, nullptr, 0u, kind == 0 ? layer : kGone, kind == 1 ? layer : kGone, r->stream));
    --layers;
    return FRT_OK;
}
int frt_renderer_remove_texture(frt_renderer* r, int kind, uint32_t layer) {
    if (const int rc = check_entry(r, "remove_texture", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_remove_texture(kind, layer, r->rf.color_layers, r->rf.data_layers, nullptr, 0, why)) return fail(rc, "remove_texture: " + why);      // (what needs no device first)
    std::vector<frt_material> mats;
    if (const int rc = read_materials(r, mats)) { if (rc == FRT_ERR_HIP) r->failed = true; return rc; }
    if (const int rc = check_remove_texture(kind, layer, r->rf.color_layers, r->rf.data_layers, mats.data(), mats.size(), why)) return fail(rc, "remove_texture: " + why);
    const int rc = remove_texture_impl(r, kind, layer);
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// ------------------------------------------------------------------------------------------------ ray queries
// Ordering: a query is enqueued on the main stream and only reads the scene replica. Every writer of the replica is on that stream too: the instance
// update and the deformation (their copies, kernels and refit levels; the ahead stream is fenced into the main stream before them), and the rebuild,
// whose kernels run there and which waits for the stream before it swaps the buffers — so the buffers a rebuild builds into are the ones that left the
// replica at the previous rebuild's wait, behind which no query can read them, and a query enqueued after the swap reads the new ones. The frame's
// own kernels on the other streams read the scene as well and write none of it. Nothing here touches frame state, counters, queues or a speculation.
enum { kQueryClosest = 0, kQueryAny = 1, kQueryPick = 2 };
static int query_impl(frt_renderer* r, int kind, const frt_camera_uniform* cam, uint32_t n, const void* in, void* out, uint32_t flags, const char* what) {
    const std::string w(what);
    if (!r) return fail(FRT_ERR_INVALID_ARG, w + ": null renderer");
    if (flags & ~FRT_QUERY_DEVICE) return fail(FRT_ERR_INVALID_ARG, w + ": unknown flag (FRT_QUERY_DEVICE)");
    if (n > kQueryMaxRays) return fail(FRT_ERR_INVALID_ARG, w + ": more than 2^26 rays in one call");
    if (const int rc = check_entry(r, w, kQuadTree)) return rc;
    if (n == 0) return FRT_OK;
    if (!in || !out || (kind == kQueryPick && !cam)) return fail(FRT_ERR_INVALID_ARG, w + ": null pointer");
    if (const int rc = check_entry(r, w, kNotFailed)) return rc;      // (a query may run while a frame is open, and needs no level ranges)
    const size_t in_bytes = (size_t)n * (kind == kQueryPick ? 8u : 32u), out_bytes = (size_t)n * (kind == kQueryAny ? 1u : 32u);
    CameraView cv{};
    if (kind == kQueryPick) memcpy(&cv, cam, sizeof(cv));
    auto launch = [&](const void* d_in, void* d_out) {
        // (vote and wg_rows as they are NOW: a rebuild changes both with the tree)
        if (kind == kQueryClosest) return launch_query_closest(r->sv, r->vote, r->wg_rows, n, d_in, d_out, r->stream);
        if (kind == kQueryAny) return launch_query_any(r->sv, r->vote, r->wg_rows, n, d_in, d_out, r->stream);
        return launch_query_pick(r->sv, r->vote, r->wg_rows, cv, r->W, r->H, n, d_in, d_out, r->stream);
    };
    if (flags & FRT_QUERY_DEVICE) {
        if (((uintptr_t)in & 15u) || (kind != kQueryAny && ((uintptr_t)out & 15u))) return fail(FRT_ERR_INVALID_ARG, w + ": device pointers must be 16-byte aligned");
        FRT_DEVICE(r);
        HIP_TRY(launch(in, out));
        return FRT_OK;
    }
    if (kind == kQueryPick) {
        const uint32_t* xy = static_cast<const uint32_t*>(in);
        for (uint32_t k = 0; k < n; ++k)
            if (xy[2 * (size_t)k] >= r->W || xy[2 * (size_t)k + 1] >= r->H)
                return fail(FRT_ERR_INVALID_ARG, w + ": pixel (" + std::to_string(xy[2 * (size_t)k]) + ", " + std::to_string(xy[2 * (size_t)k + 1]) + ") is outside the " +
                                                     std::to_string(r->W) + " x " + std::to_string(r->H) + " frame");
    }
    FRT_DEVICE(r);
    Staging& q = r->qry;
    const size_t out_at = (in_bytes + 255u) & ~(size_t)255u, all_bytes = out_at + out_bytes;
    if (const int rc = q.reserve(all_bytes, all_bytes, r->stream)) return rc;      // (never marked: the call waits for its own copies below)
    memcpy(q.h, in, in_bytes);
    HIP_TRY(hipMemcpyAsync(q.d, q.h, in_bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch(q.d, q.d + out_at));
    HIP_TRY(hipMemcpyAsync(q.h + out_at, q.d + out_at, out_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    memcpy(out, q.h + out_at, out_bytes);
    return FRT_OK;
}
int frt_renderer_trace_closest(frt_renderer* r, uint32_t n, const frt_ray* rays, frt_ray_hit* out, uint32_t flags) {
    return query_impl(r, kQueryClosest, nullptr, n, rays, out, flags, "trace_closest");
}
int frt_renderer_trace_any(frt_renderer* r, uint32_t n, const frt_ray* rays, uint8_t* occluded_out, uint32_t flags) {
    return query_impl(r, kQueryAny, nullptr, n, rays, occluded_out, flags, "trace_any");
}
int frt_renderer_pick(frt_renderer* r, const frt_camera_uniform* cam, uint32_t n, const uint32_t* xy, frt_ray_hit* out, uint32_t flags) {
    return query_impl(r, kQueryPick, cam, n, xy, out, flags, "pick");
}

int frt_renderer_tree_stats(frt_renderer* r, uint32_t st[4]) {
    if (!r || !st) return fail(FRT_ERR_INVALID_ARG, "renderer tree_stats: null");
    st[0] = r->sv.num_nodes4; st[1] = r->wg_rows > 0u ? r->wg_rows - 1u : 0u;
    st[2] = r->rf.quad_levels.empty() ? 0u : (uint32_t)r->rf.quad_levels.size() - 1u; st[3] = r->rbt.done ? r->rbt.origin : 0u;
    return FRT_OK;
}
int frt_renderer_rebuild_stats(frt_renderer* r, uint32_t st[4]) {
    if (!r || !st) return fail(FRT_ERR_INVALID_ARG, "renderer rebuild_stats: null");
    for (int k = 0; k < 4; ++k) st[k] = r->rbt.last[k];
    return FRT_OK;
}
int frt_renderer_read_scene(frt_renderer* r, int which, void* out) {
    if (!r || !out) return fail(FRT_ERR_INVALID_ARG, "read_scene: null");
    const SceneView& sv = r->sv;
    const void* src = nullptr; size_t bytes = 0;
    switch (which) {
    case 2: src = sv.materials; bytes = (size_t)sv.num_materials * sizeof(MaterialView); break;
    case 3: src = sv.lights; bytes = (size_t)sv.num_lights * sizeof(LightView); break;
    case 4: src = sv.attributes; bytes = (size_t)pool_verts(r) * sizeof(VertexAttrView); break;
    case 5: src = sv.indices; bytes = (size_t)pool_indices(r) * sizeof(uint32_t); break;
    case 6: src = sv.mesh_infos; bytes = r->rf.mesh_tris.size() * sizeof(MeshInfoView); break;
    case 18: {      // (made at the first call that needs them: frt_renderer_add_instances, _add_meshes, or this one)
        FRT_DEVICE(r);
        if (const int rc = sync_all(r)) return rc;
        if (const int rc = ensure_normals(r)) return rc;
        src = r->ie.d_normals; bytes = (size_t)pool_verts(r) * sizeof(float4);
    } break;
    case 10: src = sv.nodes4; bytes = (size_t)sv.num_nodes4 * sizeof(QuadNode); break;
    case 13: src = sv.tris; bytes = (size_t)sv.num_tris * sizeof(TriSlot); break;
    case 15:
        if (r->rbt.done) return fail(FRT_ERR_STATE, "read_scene: the pair tree is not rebuilt by frt_renderer_rebuild_tree and no longer describes the replica");
        src = sv.nodes; bytes = (size_t)sv.num_nodes * sizeof(PairNode); break;
    case 16: src = sv.instances; bytes = r->rf.inst.size() * sizeof(InstanceDev); break;
    case 17: src = sv.shade_tris; bytes = (size_t)sv.num_tris * sizeof(ShadeTri); break;
    default: return fail(FRT_ERR_INVALID_ARG, "read_scene: unknown selector (2 - 6, 10, 13, 15 - 18)");
    }
    FRT_DEVICE(r);
    { int rc = sync_all(r); if (rc) return rc; }
    if (bytes) HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return FRT_OK;
}

} // extern "C"
