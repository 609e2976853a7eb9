// frt_scene_edit.hip — every call that edits a renderer's scene replica between frames (include/frt.h), host code only:
//   moving instances, deforming, skinning and morphing meshes, the rebuild  DESIGN.md §11
//   the material, light and texture edits                                   §13
//   adding and removing instances                                           §14
//   new meshes, materials, texture layers and lights                        §15
//   removing meshes, materials, layers and lights                           §16
// The calls that only read the replica (the ray queries, frt_renderer_read_scene, the statistics and counts) are in frt_scene_read.hip; the kernels in
// frt_refit.hip, frt_refit_device.hip, frt_deform.hip, frt_pose_batch.hip, frt_material_edit.hip, frt_instance_edit.hip, frt_mesh_edit.hip, frt_scene_remove.hip, frt_rebuild.hip and frt_ploc.hip.
//
// All edits share one scheme:
//   - the call frame (edit_frame): the device guard, the stream order behind the finished frames, the body, `failed` on a HIP error;
//   - capacities (PoolState::cap, pool_count, pool_cap, reserve_pools): every buffer of the replica that is sized by a count;
//   - the buffers beside the replica that a call writes and that then trade places with the replica's (OwnedBuf);
//   - staging (Staging): what a call uploads goes through a pinned block that is reused once the copies out of it have completed.
// The seven calls on meshes are one family: one entry check (check_mesh_call), one check of a device pointer (check_device_input), one type and one
// helper for what a bind call leaves with a mesh (RefitState::MeshBinding, bind_to_mesh), and two bodies. frt_renderer_set_mesh_vertices runs
// deform_mesh (a DeformCall says where the positions are, a DeformLayout where each section of the call's blocks lies; two steps, stage and apply).
// Everything that poses runs pose_meshes over the segmented kernels of frt_pose_batch.hpp: frt_renderer_set_mesh_poses, the batch over several
// meshes, and the three single-mesh posing calls, each a batch of one behind its own checks.
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
    f.pos_offset.clear(); f.index_offset.clear(); f.vert_count.clear(); f.attr_offset.clear(); f.mesh_tris.clear(); f.adj.clear();
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
// one is in flight); here they do, as the edit calls always did: one wait on an idle stream, and only at a call that grows the block.
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
int Staging::upload(const void* src, size_t bytes, hipStream_t stream) {
    if (const int rc = reserve(bytes, bytes, stream)) return rc;
    memcpy(h, src, bytes);
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream));
    return mark(stream);
}
void Staging::release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (ev) (void)hipEventDestroy(ev);
    *this = Staging();
}

// ------------------------------------------------------------------------------------------------ the call frame
#if FRT_EXPERIMENTS
// lib/libfrt_exp.so only: do this renderer's kernels walk the product's quad tree? That is the tree a refit, a rebuild and a query work on; the 8-wide tree,
// the quantized pair nodes of the resident kernels and the pair tree of the compacting, wavefront, stream and refill kernels are not kept up with it.
static bool walks_quad_tree(const frt_renderer* r) {
    return !(r->walk == kWalkWide || r->walk == kWalkWideLds || r->x.resident || (r->flags & FRT_FLAG_COMPACTION) || r->x.wavefront || r->x.stream_mode || r->x.refill);
}
#endif
int frt::check_entry(const frt_renderer* r, const std::string& what, unsigned parts) {
    if (!r) return fail(FRT_ERR_INVALID_ARG, what + ": null");
    if ((parts & kNotFailed) && r->failed) return fail(FRT_ERR_STATE, what + ": an earlier frame failed in the middle of its stages; call frt_renderer_clear");
    if ((parts & kBetweenFrames) && r->frame_open) return fail(FRT_ERR_STATE, what + ": a frame is open (call it between frames)");
    if ((parts & kRefit) && !r->rf.ok) return fail(FRT_ERR_STATE, what + ": the scene's trees are not numbered breadth-first");
#if FRT_EXPERIMENTS
    if ((parts & kQuadTree) && !walks_quad_tree(r)) return fail(FRT_ERR_INVALID_ARG, what + ": this renderer's kernels do not walk the quad tree, the only tree this call keeps up or reads");
#endif
    return FRT_OK;
}
std::string frt::check_posed_meshes(const frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, bool skin, const void* palette, uint32_t njoints, bool morph, const void* weights, uint32_t ntargets, bool host_memory) {
    const RefitState& f = r->rf;
    std::string bad = check_pose_batch(n, mesh_ids, f.vert_count.size(), skin, morph);
    for (uint32_t k = 0; k < n && bad.empty(); ++k) {
        const uint32_t m = mesh_ids[k];
        if (skin) bad = check_mesh_pose(static_cast<const float*>(palette), njoints, m < f.skins.size() ? f.skins[m].count : 0u, host_memory && k == 0);
        if (morph && bad.empty()) bad = check_mesh_morph_weights(static_cast<const float*>(weights), ntargets, m < f.morphs.size() ? f.morphs[m].count : 0u, host_memory && k == 0);
        if (!bad.empty()) bad = "mesh " + std::to_string(m) + ": " + bad;
    }
    return bad;
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
// What every edit runs its `body` in, once its arguments are checked: the renderer's device current, the main stream ordered behind the finished frames
// (`drop`: the speculation dropped, see above; only the rebuild keeps it), and a renderer whose HIP call failed marked as failed. A composite call runs
// the bodies of its parts inside one frame.
template <class Body>
static int edit_frame(frt_renderer* r, bool drop, Body body) {
    DeviceGuard guard(r->device);
    int rc = guard.ok ? order_behind_frames(r, drop) : fail(FRT_ERR_HIP, "hipSetDevice failed");
    if (rc == FRT_OK) rc = body();
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// ------------------------------------------------------------------------------------------------ capacities and owned buffers
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
int OwnedBuf::ensure(frt_renderer* r, size_t need) {
    if (p && bytes >= need) return FRT_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));      // (a kernel of an earlier call may still read what is freed)
    scene_free(r, p);
    p = nullptr; bytes = 0;
    if (const int rc = scene_alloc(r, need, &p)) return rc;
    bytes = need;
    return FRT_OK;
}
void OwnedBuf::release(frt_renderer* r) {
    if (!p) return;
    (void)hipStreamSynchronize(r->stream);
    scene_free(r, p);
    p = nullptr; bytes = 0;
}

uint32_t frt::pool_count(const frt_renderer* r, int pool) {
    const RefitState& f = r->rf;
    switch (pool) {
    case kPoolVerts: return f.attr_offset.empty() ? 0u : f.attr_offset.back() + f.vert_count.back();
    case kPoolIndices: return f.index_offset.empty() ? 0u : f.index_offset.back() + 3u * f.mesh_tris.back();
    case kPoolMeshes: return (uint32_t)f.mesh_tris.size();
    case kPoolMaterials: return r->sv.num_materials;
    case kPoolLights: return r->sv.num_lights;
    case kPoolColor: return f.color_layers;
    case kPoolData: return f.data_layers;
    case kPoolTris: return r->sv.num_tris;
    default: return (uint32_t)f.inst.size();
    }
}
static uint32_t pool_cap(const frt_renderer* r, int p) { return r->pools.cap[p] ? r->pools.cap[p] : pool_count(r, p); }
static void pin_capacity(frt_renderer* r, int p) { r->pools.cap[p] = pool_cap(r, p); }      // before the count moves: the buffers keep their room
// The replica's buffer `live` (the caller's pointer of whatever type, `elem` bytes per element) gets room for `cap` elements: a new allocation, a
// device-to-device copy of the `used` in use, the old one freed. `oom`: what an allocation that fails is, FRT_ERR_LIMIT (nothing has changed) or FRT_ERR_HIP.
static int grow_buffer(frt_renderer* r, const void* live_ptr, size_t elem, size_t used, size_t cap, int oom) {
    const void** live = static_cast<const void**>(const_cast<void*>(live_ptr));
    void* d = nullptr;
    const hipError_t e = hipMalloc(&d, std::max<size_t>(cap * elem, 16));
    if (e != hipSuccess && oom == FRT_ERR_LIMIT) {
        (void)hipGetLastError();
        return fail(FRT_ERR_LIMIT, "no device memory for " + std::to_string(cap * elem) + " bytes (nothing changed)");
    }
    HIP_TRY(e);
    r->scene_allocs.push_back(d);
    if (used) HIP_TRY(hipMemcpy(d, *live, used * elem, hipMemcpyDeviceToDevice));
    scene_free(r, *live);
    *live = d;
    return FRT_OK;
}
// Room for `need[pool]` elements in every pool (0: the pool is not asked about). Nothing happens while the capacities suffice. A pool that is too small
// grows behind one wait for the stream: every buffer of the replica that is sized by it is replaced (grow_buffer). Capacities at least double (the
// texture arrays, 4 MiB a layer: grown_layer_capacity) and are never shrunk. The pools of §15 refuse with FRT_ERR_LIMIT when the device has no memory
// left; for the triangles and instances that is a HIP error, as every failure of the calls of §14 past their checks.
static int reserve_pools(frt_renderer* r, const uint32_t need[kPoolCount]) {
    PoolState& e = r->pools;
    SceneView& sv = r->sv;
    bool synced = false, grew = false;
    for (int p = 0; p < kPoolCount; ++p) {
        const uint32_t used = pool_count(r, p), have = pool_cap(r, p);
        if (need[p] <= have) continue;
        if (!synced) { HIP_TRY(hipStreamSynchronize(r->stream)); synced = true; }      // (the ahead stream is fenced into it: no kernel reads what is replaced below)
        const uint32_t cap = p == kPoolColor || p == kPoolData ? grown_layer_capacity(have, need[p])
                           : grown_capacity(have, need[p], p == kPoolMaterials ? kMaxMaterials : p == kPoolTris ? kMaxSceneTris : kMaxPoolElems);
        const int oom = p < kPoolTris ? FRT_ERR_LIMIT : FRT_ERR_HIP;
        auto grow = [&](const void* live_ptr, size_t elem) { return grow_buffer(r, live_ptr, elem, used, cap, oom); };
        int rc = FRT_OK;
        switch (p) {
        case kPoolVerts:
            if ((rc = grow(&r->rf.d_pos, sizeof(float4)))) return rc;
            if ((rc = grow(&sv.attributes, sizeof(VertexAttrView)))) return rc;
            rc = grow(&e.d_normals, sizeof(float4));
            break;
        case kPoolIndices: rc = grow(&sv.indices, sizeof(uint32_t)); break;
        case kPoolMeshes: rc = grow(&sv.mesh_infos, sizeof(MeshInfoView)); break;
        case kPoolMaterials: rc = grow(&sv.materials, sizeof(MaterialView)); break;
        case kPoolLights: rc = grow(&sv.lights, sizeof(LightView)); break;
        case kPoolColor: rc = grow(&sv.color_tex, kTextureLayerBytes); break;
        case kPoolData: rc = grow(&sv.data_tex, kTextureLayerBytes); break;
        case kPoolTris:
            if ((rc = grow(&sv.tris, sizeof(TriSlot)))) return rc;
            if ((rc = grow(&sv.shade_tris, sizeof(ShadeTri)))) return rc;
            rc = grow(&r->rf.d_slot_of, sizeof(uint32_t));
            break;
        default: rc = grow(&sv.instances, sizeof(InstanceView)); break;
        }
        if (rc) return rc;
        e.cap[p] = cap;
        grew = grew || p < kPoolTris;      // (frt_renderer_pool_counts reports the growths of the pools of §15)
    }
    if (grew) ++e.growths;
    return FRT_OK;
}
// The decoded normal of every vertex of the replica, made once, at the first call that needs them: the attributes come back from the device (a
// deformation may have replaced them) and are decoded by the function build_gpu_layout uses. With room for the vertex pool's capacity.
int frt::ensure_normals(frt_renderer* r) {
    if (r->pools.d_normals) return FRT_OK;
    const size_t nverts = pool_count(r, kPoolVerts);
    std::vector<frt_vertex_attr> attrs(nverts);
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (nverts) HIP_TRY(hipMemcpy(attrs.data(), r->sv.attributes, nverts * sizeof(frt_vertex_attr), hipMemcpyDeviceToHost));
    std::vector<float> nrm(4 * nverts, 0.0f);
    for (size_t v = 0; v < nverts; ++v) decoded_vertex_normal(attrs[v], &nrm[4 * v]);
    void* d = nullptr;
    if (const int rc = scene_alloc(r, (size_t)pool_cap(r, kPoolVerts) * sizeof(float4), &d)) return rc;
    if (nverts) HIP_TRY(hipMemcpy(d, nrm.data(), nrm.size() * sizeof(float), hipMemcpyHostToDevice));
    r->pools.d_normals = static_cast<const float4*>(d);
    return FRT_OK;
}

// ------------------------------------------------------------------------------------------------ the tables of the device-input transforms
// RefitState::inst[].m, .w2o and .flip are current afterwards: after a device-input set_instance_transforms the truth is the matrix table on the device,
// which is read back here, once, behind a wait for the stream. Every call that reads a mirrored matrix (or is about to replace the tables) begins with this.
static int sync_matrix_mirror(frt_renderer* r) {
    RefitState& f = r->rf;
    DeviceTransformState& x = f.xf;
    if (!x.mirror_stale) return FRT_OK;
    std::vector<float> m(16 * f.inst.size());
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (!m.empty()) HIP_TRY(hipMemcpy(m.data(), x.m.p, m.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < f.inst.size(); ++i) {
        InstanceRec& in = f.inst[i];
        if (!memcmp(in.m, &m[16 * i], sizeof(in.m))) continue;
        memcpy(in.m, &m[16 * i], sizeof(in.m));
        instance_inverse(in.m, in.w2o, in.flip);
    }
    x.mirror_stale = false;
    return FRT_OK;
}
// An edit has changed what the table of per-instance constants restates (`matrices`: and the mirror, which is current, no longer equals the matrix table):
// the next device-input call uploads them again.
static void drop_transform_tables(frt_renderer* r, bool matrices) {
    r->rf.xf.consts_ok = false;
    if (matrices) r->rf.xf.m_ok = false;
}
// The two words a device-input call's kernels report through exist afterwards, zeroed when made: [0] the flag of the call in flight, [1] the calls
// rejected so far (RefitState::d_reject, DeviceTransformState::d_reject).
static int ensure_reject_words(frt_renderer* r, uint32_t*& words) {
    if (words) return FRT_OK;
    void* d = nullptr;
    if (const int rc = scene_alloc(r, 2 * sizeof(uint32_t), &d)) return rc;
    HIP_TRY(hipMemset(d, 0, 2 * sizeof(uint32_t)));
    words = static_cast<uint32_t*>(d);
    return FRT_OK;
}
// The tables of a device-input call exist and are current afterwards; what is not is uploaded from the host's bookkeeping on the main stream.
static int ensure_transform_tables(frt_renderer* r) {
    RefitState& f = r->rf;
    DeviceTransformState& x = f.xf;
    int rc;
    if ((rc = ensure_reject_words(r, x.d_reject))) return rc;
    if (x.consts_ok && x.m_ok) return FRT_OK;
    const size_t ni = f.inst.size(), cap = std::max<size_t>(pool_cap(r, kPoolInstances), ni);
    if (x.m.bytes < cap * 64u) {      // (a table that is replaced loses its contents: the matrices come from the mirror)
        if ((rc = sync_matrix_mirror(r))) return rc;
        x.m_ok = false;
    }
    if ((rc = x.consts.ensure(r, cap * sizeof(InstanceConst)))) return rc;
    if ((rc = x.m.ensure(r, cap * 64u))) return rc;
    if ((rc = x.last.ensure(r, cap * sizeof(uint32_t)))) return rc;
    const size_t const_bytes = x.consts_ok ? 0 : ni * sizeof(InstanceConst), m_bytes = x.m_ok ? 0 : ni * 64u;
    if ((rc = x.up.reserve(const_bytes + m_bytes, 0, r->stream))) return rc;
    if (const_bytes) {
        InstanceConst* c = reinterpret_cast<InstanceConst*>(x.up.h);
        for (size_t i = 0; i < ni; ++i) {
            const InstanceRec& in = f.inst[i];
            memset(&c[i], 0, sizeof(c[i]));
            c[i].first_tri = in.first_tri; c[i].tri_count = in.tri_count; c[i].index_offset = f.index_offset[in.mesh_id]; c[i].pos_offset = f.pos_offset[in.mesh_id];
            c[i].mesh_id = in.mesh_id; c[i].mat_id = in.mat_id; c[i].light = 0xFFFFFFFFu; c[i].light_kind = in.light_kind;
            if (in.light >= 0 && (size_t)in.light < f.lights.size()) { c[i].light = (uint32_t)in.light; memcpy(c[i].emission, f.lights[(size_t)in.light].emission, 16); }
        }
        HIP_TRY(hipMemcpyAsync(x.consts.p, x.up.h, const_bytes, hipMemcpyHostToDevice, r->stream));
    }
    if (m_bytes) {
        float* m = reinterpret_cast<float*>(x.up.h + const_bytes);
        for (size_t i = 0; i < ni; ++i) memcpy(m + 16 * i, f.inst[i].m, 64);
        HIP_TRY(hipMemcpyAsync(x.m.p, x.up.h + const_bytes, m_bytes, hipMemcpyHostToDevice, r->stream));
    }
    if (const_bytes + m_bytes) if ((rc = x.up.mark(r->stream))) return rc;
    x.consts_ok = x.m_ok = true;
    return FRT_OK;
}

extern "C" {

// ------------------------------------------------------------------------------------------------ moving instances
// Is `p` device memory of the renderer's device, `align`-byte aligned, with `bytes` bytes of its allocation behind it? (What a kernel would otherwise
// find out by faulting.) `call`, `flag`: the names the message begins and ends with.
static int check_device_pointer(const frt_renderer* r, const void* p, size_t bytes, size_t align, const char* call, const char* what, const char* flag) {
    const std::string w = std::string(call) + ": " + what;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return fail(FRT_ERR_INVALID_ARG, w + " are not device memory (" + flag + ")"); }
    if (at.type != hipMemoryTypeDevice || at.device != r->device)
        return fail(FRT_ERR_INVALID_ARG, w + " are not memory of the renderer's device " + std::to_string(r->device) + " (" + flag + ")");
    if ((uintptr_t)p & (align - 1u)) return fail(FRT_ERR_INVALID_ARG, w + ": device pointers must be " + std::to_string(align) + "-byte aligned");
    hipDeviceptr_t base = nullptr; size_t size = 0;      // the allocation around p holds `bytes` from p on
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return fail(FRT_ERR_INVALID_ARG, w + ": no device allocation holds the pointer"); }
    const size_t before = (size_t)((const uint8_t*)p - (const uint8_t*)base);
    if (before > size || size - before < bytes)
        return fail(FRT_ERR_INVALID_ARG, w + ": the device allocation holds " + std::to_string(size - std::min(before, size)) + " bytes from the pointer on, " + std::to_string(bytes) + " are needed");
    return FRT_OK;
}
// The same with the renderer's device current, as the pointer queries need it: what every call that takes device input asks of each of its pointers.
static int check_device_input(const frt_renderer* r, const void* p, size_t bytes, size_t align, const char* call, const char* what, const char* flag = "FRT_DEFORM_DEVICE") {
    DeviceGuard guard(r->device);
    if (!guard.ok) return fail(FRT_ERR_HIP, "hipSetDevice failed");
    return check_device_pointer(r, p, bytes, align, call, what, flag);
}
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
int frt_renderer_set_instance_transforms(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* mats) {
    if (const int rc = check_entry(r, "set_instance_transforms", kEditChecks | kRefit)) return rc;
    const std::string bad = check_instance_transforms(n, ids, mats, r->rf.inst.size());
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: " + bad);
    return edit_frame(r, true, [&]() -> int {
        RefitState& f = r->rf;
        if (n == 0) return FRT_OK;      // (behind the fence: an empty call still drops the speculation)
        if (const int rc = sync_matrix_mirror(r)) return rc;      // (after device-input calls: the mirror written below is the truth again)
        f.xf.m_ok = false;
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
        if (const int rc = f.rec.upload(rec.data(), rec.size() * sizeof(MovedInstance), r->stream)) return rc;
        RefitArgs a{reinterpret_cast<const MovedInstance*>(f.rec.d), (uint32_t)rec.size(), work, f.d_pos, f.d_slot_of, const_cast<unsigned int*>(f.d_ext)};
        HIP_TRY(launch_instance_transform(r->sv, a, r->stream));
        return refit_levels(r);
    });
}
// The body of a device-input call, behind ensure_transform_tables: n >= 1 records in device memory through the launches of frt_refit_device.hpp. The
// scene extent and the refit follow in the caller (refit_scene), once.
static int transform_instances_device(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* mats) {
    RefitState& f = r->rf;
    DeviceTransformState& x = f.xf;
    const TransformInput a{ids, reinterpret_cast<const float4*>(mats), n, (uint32_t)f.inst.size(), x.consts.as<InstanceConst>(), x.m.as<float4>(), x.last.as<uint32_t>(), x.d_reject,
                           f.d_pos, f.d_slot_of, pool_cap(r, kPoolVerts), pool_cap(r, kPoolIndices)};
    HIP_TRY(launch_device_transforms(r->sv, a, r->stream));
    x.mirror_stale = true;      // (a rejected call leaves the table as it was: reading it back then changes nothing)
    return FRT_OK;
}
// What follows a body that wrote triangles, once per call: the scene extent and both trees refit.
static int refit_scene(frt_renderer* r) {
    HIP_TRY(launch_scene_extent(r->sv, const_cast<unsigned int*>(r->rf.d_ext), r->stream));
    return refit_levels(r);
}
// Device input (FRT_TRANSFORM_DEVICE): nothing of the call's data is seen by the host. The entry checks, the stream order and the dropped speculation are
// the host form's; the kernels of frt_refit_device.hpp do the rest from the renderer's device tables, and the host's mirror of the matrices goes stale.
static const uint32_t kMaxDeviceTransforms = 1u << 26;
int frt_renderer_set_instance_transforms_ex(frt_renderer* r, uint32_t n, const uint32_t* ids, const float* mats, uint32_t flags) {
    if (const int rc = check_entry(r, "set_instance_transforms", kEditChecks | kRefit)) return rc;
    if (flags & ~FRT_TRANSFORM_DEVICE) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: unknown flag bits");
    if (!(flags & FRT_TRANSFORM_DEVICE)) return frt_renderer_set_instance_transforms(r, n, ids, mats);
    if (n > 0 && (!ids || !mats)) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: null ids or matrices");
    if (n > kMaxDeviceTransforms) return fail(FRT_ERR_INVALID_ARG, "set_instance_transforms: more than 2^26 records in one device-input call");
    if (n > 0) {
        if (const int rc = check_device_input(r, ids, (size_t)n * 4, 4, "set_instance_transforms", "ids", "FRT_TRANSFORM_DEVICE")) return rc;
        if (const int rc = check_device_input(r, mats, (size_t)n * 64, 16, "set_instance_transforms", "matrices", "FRT_TRANSFORM_DEVICE")) return rc;
    }
    return edit_frame(r, true, [&]() -> int {
        if (n == 0) return FRT_OK;
        if (const int rc = ensure_transform_tables(r)) return rc;
        if (const int rc = transform_instances_device(r, n, ids, mats)) return rc;
        return refit_scene(r);
    });
}

// ------------------------------------------------------------------------------------------------ the mesh-edit family ("Deforming meshes", "Skinning", "Morph targets")
// What each of the seven calls checks first, in this order: the entry, flag bits outside `allowed_flags`, the mesh id.
static int check_mesh_call(const frt_renderer* r, const char* call, uint32_t mesh_id, uint32_t flags, uint32_t allowed_flags) {
    const std::string c(call);
    if (const int rc = check_entry(r, c, kEditChecks | kRefit)) return rc;
    if (flags & ~allowed_flags) return fail(FRT_ERR_INVALID_ARG, c + ": unknown flag bits");
    if (mesh_id >= r->rf.vert_count.size())
        return fail(FRT_ERR_INVALID_ARG, c + ": mesh id " + std::to_string(mesh_id) + " out of range (" + std::to_string(r->rf.vert_count.size()) + " meshes)");
    return FRT_OK;
}
static const uint32_t kDeformFlags = FRT_DEFORM_RECOMPUTE_NORMALS | FRT_DEFORM_DEVICE;

// The vertex -> corner adjacency of mesh `m` is on the device afterwards (RefitState::adj). Made once per mesh from the replica's own indices: a wait for
// the stream and one read-back, as ensure_normals; frt_renderer_remove_meshes keeps the list in step with the mesh ids.
static int ensure_adjacency(frt_renderer* r, uint32_t m) {
    RefitState& f = r->rf;
    if (f.adj.size() < f.mesh_tris.size()) f.adj.resize(f.mesh_tris.size(), nullptr);
    if (f.adj[m]) return FRT_OK;
    const uint32_t nidx = 3u * f.mesh_tris[m], nverts = f.vert_count[m];
    std::vector<uint32_t> idx(nidx), off, corners;
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (nidx) HIP_TRY(hipMemcpy(idx.data(), r->sv.indices + f.index_offset[m], (size_t)nidx * 4, hipMemcpyDeviceToHost));
    build_vertex_corners(idx.data(), nidx, nverts, off, corners);
    off.insert(off.end(), corners.begin(), corners.end());
    void* d = nullptr;
    if (const int rc = scene_alloc(r, off.size() * 4, &d)) return rc;
    HIP_TRY(hipMemcpy(d, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    f.adj[m] = static_cast<const uint32_t*>(d);
    return FRT_OK;
}

// One frt_renderer_set_mesh_vertices_ex, as the call has checked it. `pos4` and `attrs` (which live where the positions live) are the caller's host
// memory or, `on_device` (FRT_DEFORM_DEVICE), the caller's device memory.
struct DeformCall {
    uint32_t mesh_id = 0, nverts = 0;
    bool on_device = false;                       // the positions reach the replica through frt_deform.hpp's validation and copy-in
    bool recompute = false;                       // FRT_DEFORM_RECOMPUTE_NORMALS
    const float* pos4 = nullptr;
    const frt_vertex_attr* attrs = nullptr;
    bool shade() const { return attrs || recompute; }                    // the shading records are written again: the device block holds decoded normals
    bool host_decode() const { return attrs && !recompute && !on_device; }      // ... which the host decodes from the call's attributes
};
// Where everything a call stages lies in the two blocks of RefitState::def, computed once; a section that a call does not use is empty.
//   pinned: positions | attributes | instance records | decoded normals
//   device:                          instance records | decoded normals
// The first two pinned sections are copied into the replica (the object-space positions the instance update reads, SceneView::attributes). Records and
// normals are neighbours in both blocks and go over in one copy (`h_up`); the device's normals section is there whenever shading records are written
// (the normal pass fills it where the host did not), the pinned one only for the host's decode.
struct Section { size_t off = 0, bytes = 0; };
struct DeformLayout {
    Section h_pos, h_attrs, h_rec, h_nrm, h_up, d_rec, d_nrm;
    size_t h_total = 0, d_total = 0;
    DeformLayout(const DeformCall& c, size_t ninstances) {
        auto put = [](size_t& total, size_t bytes) { const Section s{total, bytes}; total += bytes; return s; };
        const size_t n = c.nverts, rec = ninstances * sizeof(DeformInstance);
        h_pos = put(h_total, c.on_device ? 0 : n * 16);
        h_attrs = put(h_total, c.attrs && !c.on_device ? n * sizeof(frt_vertex_attr) : 0);
        h_rec = put(h_total, rec);
        h_nrm = put(h_total, c.host_decode() ? n * 16 : 0);
        h_up = Section{h_rec.off, h_rec.bytes + h_nrm.bytes};
        d_rec = put(d_total, rec);
        d_nrm = put(d_total, c.shade() ? n * 16 : 0);
    }
};
// Step 1: the call's data into the pinned block and, in stream order, out of it. RefitState::def is reused in stream order and replaced, after a wait
// for the stream, only when it has to grow.
static int stage_deform(frt_renderer* r, const DeformCall& c, const DeformLayout& l, const std::vector<DeformInstance>& rec) {
    RefitState& f = r->rf;
    const uint32_t m = c.mesh_id, cap_verts = pool_cap(r, kPoolVerts);
    if (const int rc = f.def.reserve(l.h_total, l.d_total, r->stream)) return rc;
    if ((uint64_t)f.pos_offset[m] + c.nverts > cap_verts || (uint64_t)f.attr_offset[m] + c.nverts > cap_verts)
        return fail(FRT_ERR_STATE, "set_mesh_vertices: the mesh does not lie inside the vertex pool");
    if ((uint64_t)f.index_offset[m] + 3ull * f.mesh_tris[m] > pool_cap(r, kPoolIndices))
        return fail(FRT_ERR_STATE, "set_mesh_vertices: the mesh does not lie inside the index pool");
    uint8_t* h = f.def.h; uint8_t* d = f.def.d;
    float4* pool_normals = const_cast<float4*>(r->pools.d_normals);      // (what a later frt_renderer_add_instances of this mesh reads, §14; may be null)
    if (l.h_pos.bytes) memcpy(h + l.h_pos.off, c.pos4, l.h_pos.bytes);
    if (l.h_attrs.bytes) memcpy(h + l.h_attrs.off, c.attrs, l.h_attrs.bytes);
    if (c.host_decode()) {
        float* nrm = reinterpret_cast<float*>(h + l.h_nrm.off);
        for (uint32_t v = 0; v < c.nverts; ++v) { decoded_vertex_normal(c.attrs[v], nrm + 4 * (size_t)v); nrm[4 * (size_t)v + 3] = 0.0f; }
    }
    if (l.h_rec.bytes) memcpy(h + l.h_rec.off, rec.data(), l.h_rec.bytes);
    if (!c.on_device) HIP_TRY(hipMemcpyAsync(const_cast<float4*>(f.d_pos) + f.pos_offset[m], h + l.h_pos.off, l.h_pos.bytes, hipMemcpyHostToDevice, r->stream));
    if (l.h_attrs.bytes) HIP_TRY(hipMemcpyAsync(const_cast<VertexAttrView*>(r->sv.attributes) + f.attr_offset[m], h + l.h_attrs.off, l.h_attrs.bytes, hipMemcpyHostToDevice, r->stream));
    if (l.h_up.bytes) HIP_TRY(hipMemcpyAsync(d + l.d_rec.off, h + l.h_up.off, l.h_up.bytes, hipMemcpyHostToDevice, r->stream));
    if (c.host_decode() && pool_normals) HIP_TRY(hipMemcpyAsync(pool_normals + f.attr_offset[m], h + l.h_nrm.off, l.h_nrm.bytes, hipMemcpyHostToDevice, r->stream));
    return f.def.mark(r->stream);
}
// Step 2: the caller's device positions through the validation and copy-in launches of frt_deform.hpp, the normal pass, the mesh's triangles under
// every instance of it, the scene extent and the refit. `work`: the triangles of those instances.
static int apply_deform(frt_renderer* r, const DeformCall& c, const DeformLayout& l, uint32_t ninstances, uint32_t work) {
    RefitState& f = r->rf;
    const uint32_t m = c.mesh_id, cap_verts = pool_cap(r, kPoolVerts);
    float4* block = c.shade() ? reinterpret_cast<float4*>(f.def.d + l.d_nrm.off) : nullptr;
    float4* pool_normals = const_cast<float4*>(r->pools.d_normals);
    const uint32_t* reject = c.on_device ? f.d_reject : nullptr;      // (host input was validated by the call: there is no flag to look at)
    if (c.on_device) {
        const bool decode = c.attrs && !c.recompute;
        DeformInput in{reinterpret_cast<const float4*>(c.pos4), reinterpret_cast<const float4*>(c.attrs), c.nverts, f.pos_offset[m], f.attr_offset[m], cap_verts,
                       const_cast<float4*>(f.d_pos), reinterpret_cast<float4*>(const_cast<VertexAttrView*>(r->sv.attributes)),
                       decode ? block : nullptr, decode ? pool_normals : nullptr, f.d_reject};
        HIP_TRY(launch_deform_input(in, r->stream));
    }
    if (c.recompute) {
        NormalArgs na{f.adj[m], f.adj[m] + (c.nverts + 1u), c.nverts, 3u * f.mesh_tris[m], f.index_offset[m], f.pos_offset[m], f.attr_offset[m],
                      cap_verts, pool_cap(r, kPoolIndices), f.d_pos, block, pool_normals, reject};
#if FRT_EXPERIMENTS
        const char* tri_pass = getenv("FRT_NORMALS_TRI_PASS");
        if (tri_pass && atoi(tri_pass) != 0) {
            if (const int rc = f.tri_normals.ensure(r, (size_t)f.mesh_tris[m] * sizeof(float4))) return rc;
            na.tri_scratch = f.tri_normals.as<float4>();
        }
#endif
        HIP_TRY(launch_vertex_normals(r->sv, na, r->stream));
    }
    if (work == 0) return FRT_OK;      // no instance of the mesh: no triangle changes
    DeformArgs a{reinterpret_cast<const DeformInstance*>(f.def.d + l.d_rec.off), ninstances, work, f.index_offset[m], f.pos_offset[m], f.attr_offset[m],
                 f.d_pos, block, f.d_slot_of, reject};
    HIP_TRY(launch_mesh_deform(r->sv, a, r->stream));
    HIP_TRY(launch_scene_extent(r->sv, const_cast<unsigned int*>(f.d_ext), r->stream));
    return refit_levels(r);
}
// What follows the checks of a deformation, inside its call frame: the instance records, what the call needs beside the staging, and the two steps.
static int deform_mesh(frt_renderer* r, const DeformCall& c) {
    RefitState& f = r->rf;
    int rc;
    if ((rc = sync_matrix_mirror(r))) return rc;      // (the instances' matrices are read below)
    std::vector<DeformInstance> rec;
    uint32_t work = 0;
    for (size_t i = 0; i < f.inst.size(); ++i) {      // in instance order
        const InstanceRec& in = f.inst[i];
        if (in.mesh_id != c.mesh_id) continue;
        DeformInstance d;
        d.id = (uint32_t)i; d.first_tri = in.first_tri; d.tri_count = in.tri_count; d.work_begin = work; work += in.tri_count;
        for (int col = 0; col < 4; ++col) for (int a = 0; a < 3; ++a) d.m[3 * col + a] = in.m[4 * col + a];
        rec.push_back(d);
    }
    const DeformLayout l(c, rec.size());
    if (c.recompute && (rc = ensure_adjacency(r, c.mesh_id))) return rc;
    if (c.on_device && (rc = ensure_reject_words(r, f.d_reject))) return rc;
    if ((rc = stage_deform(r, c, l, rec))) return rc;
    return apply_deform(r, c, l, (uint32_t)rec.size(), work);
}
int frt_renderer_set_mesh_vertices_ex(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts, uint32_t flags) {
    if (const int rc = check_mesh_call(r, "set_mesh_vertices", mesh_id, flags, kDeformFlags)) return rc;
    const bool dev = (flags & FRT_DEFORM_DEVICE) != 0;
    if (!dev) {
        const std::string bad = check_mesh_vertices(pos4, attrs, nverts, r->rf.vert_count[mesh_id]);
        if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: " + bad);
    } else {      // what check_mesh_vertices checks without reading the vertices; their finiteness is the validation launch's to check
        if (!pos4) return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: null positions");
        if (nverts != r->rf.vert_count[mesh_id])
            return fail(FRT_ERR_INVALID_ARG, "set_mesh_vertices: " + std::to_string(nverts) + " vertices given, the mesh has " + std::to_string(r->rf.vert_count[mesh_id]) + " (the topology is fixed)");
        if (const int rc = check_device_input(r, pos4, (size_t)nverts * 16, 16, "set_mesh_vertices", "positions")) return rc;
        if (attrs) if (const int rc = check_device_input(r, attrs, (size_t)nverts * sizeof(frt_vertex_attr), 16, "set_mesh_vertices", "attributes")) return rc;
    }
    DeformCall c;
    c.mesh_id = mesh_id; c.nverts = nverts; c.on_device = dev; c.recompute = (flags & FRT_DEFORM_RECOMPUTE_NORMALS) != 0;
    c.pos4 = pos4; c.attrs = attrs;
    return edit_frame(r, true, [&]() -> int { return deform_mesh(r, c); });
}
int frt_renderer_set_mesh_vertices(frt_renderer* r, uint32_t mesh_id, const float* pos4, const frt_vertex_attr* attrs, uint32_t nverts) {
    return frt_renderer_set_mesh_vertices_ex(r, mesh_id, pos4, attrs, nverts, 0u);
}

// ------------------------------------------------------------------------------------------------ binding skins and morph targets
// The binding of mesh `m` in `list` leaves (behind a wait: a pose's or a morph's kernel may still read it).
static int drop_binding(frt_renderer* r, std::vector<RefitState::MeshBinding>& list, uint32_t m) {
    if (m >= list.size() || !list[m].buf.p) return FRT_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    scene_free(r, list[m].buf.p);
    list[m] = RefitState::MeshBinding();
    return FRT_OK;
}
// Mesh `mesh_id` gets a binding in `list`: its buffer is [the mesh's positions | the host parts, in order]. The positions are copied from the replica's
// object-space positions on the stream, behind every deformation enqueued so far; the host parts go through the pinned block of `up`.
struct HostPart { const void* p; size_t bytes; };
static int bind_to_mesh(frt_renderer* r, const char* call, std::vector<RefitState::MeshBinding>& list, Staging& up, uint32_t mesh_id, uint32_t nverts,
                        std::initializer_list<HostPart> parts, uint32_t count) {
    RefitState& f = r->rf;
    if (list.size() <= mesh_id) list.resize((size_t)mesh_id + 1u);
    RefitState::MeshBinding& k = list[mesh_id];
    const size_t pos_bytes = (size_t)nverts * 16;
    size_t host_bytes = 0;
    for (const HostPart& part : parts) host_bytes += part.bytes;
    int rc;
    if ((uint64_t)f.pos_offset[mesh_id] + nverts > pool_cap(r, kPoolVerts)) return fail(FRT_ERR_STATE, std::string(call) + ": the mesh does not lie inside the vertex pool");
    k.count = 0;      // (a call that fails below leaves the mesh without the binding)
    if ((rc = k.buf.ensure(r, pos_bytes + host_bytes))) return rc;
    if ((rc = up.reserve(host_bytes, 0, r->stream))) return rc;
    size_t at = 0;
    for (const HostPart& part : parts) { memcpy(up.h + at, part.p, part.bytes); at += part.bytes; }
    if (nverts) {
        HIP_TRY(hipMemcpyAsync(k.buf.p, f.d_pos + f.pos_offset[mesh_id], pos_bytes, hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(k.buf.as<uint8_t>() + pos_bytes, up.h, host_bytes, hipMemcpyHostToDevice, r->stream));
    }
    if ((rc = up.mark(r->stream))) return rc;
    k.count = count;
    return FRT_OK;
}
// Skinning: [bind positions | weights | joints]. The speculation is kept: nothing a frame reads changes.
// `flags`: the mode the mesh is posed in (0, FRT_SKIN_DUAL_QUATERNION), kept beside the binding: the buffer is the same in either mode.
int frt_renderer_set_mesh_skin_ex(frt_renderer* r, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints, uint32_t flags) {
    if (const int rc = check_mesh_call(r, "set_mesh_skin", mesh_id, 0u, 0u)) return rc;
    if (flags & ~FRT_SKIN_DUAL_QUATERNION) return fail(FRT_ERR_INVALID_ARG, "set_mesh_skin: unknown flag bits");
    if (joints4) {
        const std::string bad = check_mesh_skin(joints4, weights4, nverts, njoints, r->rf.vert_count[mesh_id]);
        if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_skin: " + bad);
    }
    return edit_frame(r, false, [&]() -> int {
        if (!joints4) return drop_binding(r, r->rf.skins, mesh_id);
        if (const int rc = bind_to_mesh(r, "set_mesh_skin", r->rf.skins, r->rf.skin_up, mesh_id, nverts, {{weights4, (size_t)nverts * 16}, {joints4, (size_t)nverts * 8}}, njoints)) return rc;
        r->rf.skins[mesh_id].mode = flags;
        return FRT_OK;
    });
}
int frt_renderer_set_mesh_skin(frt_renderer* r, uint32_t mesh_id, const uint16_t* joints4, const float* weights4, uint32_t nverts, uint32_t njoints) {
    return frt_renderer_set_mesh_skin_ex(r, mesh_id, joints4, weights4, nverts, njoints, 0u);
}
// Morph targets: [base positions | deltas], the deltas in the caller's layout (target-major). The speculation is kept, as above.
int frt_renderer_set_mesh_morph_targets(frt_renderer* r, uint32_t mesh_id, const float* deltas3, uint32_t nverts, uint32_t ntargets) {
    if (const int rc = check_mesh_call(r, "set_mesh_morph_targets", mesh_id, 0u, 0u)) return rc;
    if (deltas3) {
        const std::string bad = check_mesh_morph_targets(deltas3, nverts, ntargets, r->rf.vert_count[mesh_id]);
        if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_morph_targets: " + bad);
    }
    return edit_frame(r, false, [&]() -> int {
        if (!deltas3) return drop_binding(r, r->rf.morphs, mesh_id);
        return bind_to_mesh(r, "set_mesh_morph_targets", r->rf.morphs, r->rf.morph_up, mesh_id, nverts, {{deltas3, (size_t)ntargets * nverts * 12}}, ntargets);
    });
}

// ------------------------------------------------------------------------------------------------ posing: skin, morph, or morph then skin ("Posing several meshes")
// What the two single-mesh calls that take morph weights check about them, in front of the call frame; with FRT_DEFORM_DEVICE their finiteness is the morph launch's.
static int check_morph_input(frt_renderer* r, const char* call, uint32_t mesh_id, const float* weights, uint32_t ntargets, bool dev) {
    const std::string bad = check_mesh_morph_weights(weights, ntargets, mesh_id < r->rf.morphs.size() ? r->rf.morphs[mesh_id].count : 0u, !dev);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, std::string(call) + ": " + bad);
    return dev ? check_device_input(r, weights, (size_t)ntargets * 4, 4, call, "morph weights") : FRT_OK;
}
// Where everything a batch stages lies in the two blocks of RefitState::def, a sibling of DeformLayout. The pinned block goes over in one copy; the
// device block has the call's decoded normals behind it (FRT_DEFORM_RECOMPUTE_NORMALS: the normal launch fills them, the triangle launch reads them).
//   pinned: segments | instance records | the records' segments | palette | weights
//   device: segments | instance records | the records' segments | palette | weights | decoded normals
struct PoseBatchLayout {
    Section seg, rec, rec_seg, pal, wt, d_nrm;
    size_t h_total = 0, d_total = 0;
    PoseBatchLayout(size_t nseg, size_t ninstances, size_t pal_bytes, size_t wt_bytes, size_t nrm_bytes) {
        auto put = [this](size_t bytes) { const Section s{h_total, bytes}; h_total += (bytes + 15u) & ~(size_t)15u; return s; };      // (every section 16-byte aligned)
        seg = put(nseg * sizeof(PoseSegment));
        rec = put(ninstances * sizeof(DeformInstance));
        rec_seg = put(ninstances * sizeof(uint32_t));
        pal = put(pal_bytes);
        wt = put(wt_bytes);
        d_nrm = Section{h_total, nrm_bytes};
        d_total = h_total + nrm_bytes;
    }
};
struct PoseBatchCall {
    const char* call = "";                                     // the C call's name: what a message begins with
    uint32_t n = 0; const uint32_t* mesh_ids = nullptr;
    const float* palette = nullptr; uint32_t njoints = 0;      // null: no skin launch
    const float* weights = nullptr; uint32_t ntargets = 0;     // null: no morph launch
    bool on_device = false, recompute = false;
    // frt_renderer_animate_cast: mesh k is posed under per_mesh[k]'s palette and weights (device memory; mesh_ids is null and per_mesh[k].mesh names
    // the mesh). `palette` [check_cols float4] and `weights` [check_nweights] are then the one range each that holds them all, on_device is set, and
    // the triangles take their matrices from the device matrix table, which the caller has made current: the host's mirror is not read.
    const CastMesh* per_mesh = nullptr;
    uint32_t check_cols = 0, check_nweights = 0;
    uint32_t mesh(uint32_t k) const { return per_mesh ? per_mesh[k].mesh : mesh_ids[k]; }
};
// What follows the checks of a batch, inside its call frame: the segment table, the instance records of every mesh of the batch, one staged copy and
// the launches of frt_pose_batch.hpp. `changed`: a triangle was written, so the scene extent and the refit have to follow (pose_meshes; apply_cast).
static int pose_meshes_body(frt_renderer* r, const PoseBatchCall& c, bool& changed) {
    RefitState& f = r->rf;
    const std::string call(c.call);
    int rc;
    changed = false;
    if (!c.per_mesh && (rc = sync_matrix_mirror(r))) return rc;      // (the instances' matrices are read below)
    const uint32_t cap_verts = pool_cap(r, kPoolVerts), cap_indices = pool_cap(r, kPoolIndices);
    std::vector<PoseSegment> seg(c.n);
    std::vector<int> seg_of_mesh(f.vert_count.size(), -1);
    uint64_t total = 0;
    uint32_t skins = 0, skins_dq = 0;
    bool any_morph = false;
    for (uint32_t k = 0; k < c.n; ++k) {
        const uint32_t m = c.mesh(k);
        if ((uint64_t)f.pos_offset[m] + f.vert_count[m] > cap_verts || (uint64_t)f.attr_offset[m] + f.vert_count[m] > cap_verts)
            return fail(FRT_ERR_STATE, call + ": mesh " + std::to_string(m) + " does not lie inside the vertex pool");
        if ((uint64_t)f.index_offset[m] + 3ull * f.mesh_tris[m] > cap_indices)
            return fail(FRT_ERR_STATE, call + ": mesh " + std::to_string(m) + " does not lie inside the index pool");
        if (c.recompute && (rc = ensure_adjacency(r, m))) return rc;
        PoseSegment& s = seg[k];
        s.vert_begin = (uint32_t)total; s.nverts = f.vert_count[m]; s.pos_offset = f.pos_offset[m]; s.attr_offset = f.attr_offset[m];
        s.index_offset = f.index_offset[m]; s.ntris = f.mesh_tris[m];
        const bool skin = c.per_mesh ? c.per_mesh[k].palette != nullptr : c.palette != nullptr, morph = c.per_mesh ? c.per_mesh[k].weights != nullptr : c.weights != nullptr;
        s.skin = skin ? static_cast<const uint8_t*>(f.skins[m].buf.p) : nullptr;
        s.morph = morph ? static_cast<const uint8_t*>(f.morphs[m].buf.p) : nullptr;
        s.adj = c.recompute ? f.adj[m] : nullptr;
        s.njoints = skin ? (c.per_mesh ? c.per_mesh[k].njoints : c.njoints) : 0u;
        s.skin_mode = skin ? f.skins[m].mode : 0u;      // the mode the mesh was bound with (set_mesh_skin_ex)
        s.ntargets = morph ? (c.per_mesh ? c.per_mesh[k].ntargets : c.ntargets) : 0u;
        s.palette = c.per_mesh ? reinterpret_cast<const float4*>(c.per_mesh[k].palette) : nullptr;      // (a batch under one palette: set below, once its place is known)
        s.weights = c.per_mesh ? c.per_mesh[k].weights : nullptr;
        if (skin) { ++skins; if (s.skin_mode == FRT_SKIN_DUAL_QUATERNION) ++skins_dq; }
        any_morph = any_morph || morph;
        seg_of_mesh[m] = (int)k;
        total += s.nverts;
        if (total > 0xFFFFFF00ull) return fail(FRT_ERR_INVALID_ARG, call + ": more than 2^32 - 256 vertices in one call");
    }
    std::vector<DeformInstance> rec;
    std::vector<uint32_t> rec_seg;
    uint64_t work = 0;
    for (size_t i = 0; i < f.inst.size(); ++i) {      // in instance order
        const InstanceRec& in = f.inst[i];
        if (in.mesh_id >= seg_of_mesh.size() || seg_of_mesh[in.mesh_id] < 0) continue;
        DeformInstance d;
        d.id = (uint32_t)i; d.first_tri = in.first_tri; d.tri_count = in.tri_count; d.work_begin = (uint32_t)work; work += in.tri_count;
        for (int col = 0; col < 4; ++col) for (int a = 0; a < 3; ++a) d.m[3 * col + a] = c.per_mesh ? 0.0f : in.m[4 * col + a];      // (a cast: the triangle launch reads the table)
        rec.push_back(d);
        rec_seg.push_back((uint32_t)seg_of_mesh[in.mesh_id]);
    }
    if (work > 0xFFFFFF00ull) return fail(FRT_ERR_INVALID_ARG, call + ": more than 2^32 - 256 triangles in one call");
    if ((rc = f.skinned.ensure(r, (size_t)total * 16))) return rc;
    const bool any_skin = skins != 0;
    if (any_skin && any_morph && (rc = f.morphed.ensure(r, (size_t)total * 16))) return rc;
    if ((rc = ensure_reject_words(r, f.d_reject))) return rc;
    const PoseBatchLayout l(c.n, rec.size(), c.palette && !c.on_device ? (size_t)c.njoints * 64 : 0, c.weights && !c.on_device ? (size_t)c.ntargets * 4 : 0,
                            c.recompute ? (size_t)total * 16 : 0);
    if ((rc = f.def.reserve(l.h_total, l.d_total, r->stream))) return rc;
    uint8_t* h = f.def.h; uint8_t* d = f.def.d;
    const float4* palette = !c.palette ? nullptr : reinterpret_cast<const float4*>(c.on_device ? reinterpret_cast<const uint8_t*>(c.palette) : d + l.pal.off);
    const float* weights = !c.weights ? nullptr : c.on_device ? c.weights : reinterpret_cast<const float*>(d + l.wt.off);
    if (!c.per_mesh) for (PoseSegment& s : seg) { s.palette = palette; s.weights = weights; }      // every segment under the one palette and the one weight vector
    memset(h, 0, l.h_total);      // (the padding between the sections is copied with them)
    memcpy(h + l.seg.off, seg.data(), l.seg.bytes);
    if (l.rec.bytes) memcpy(h + l.rec.off, rec.data(), l.rec.bytes);
    if (l.rec_seg.bytes) memcpy(h + l.rec_seg.off, rec_seg.data(), l.rec_seg.bytes);
    if (l.pal.bytes) memcpy(h + l.pal.off, c.palette, l.pal.bytes);
    if (l.wt.bytes) memcpy(h + l.wt.off, c.weights, l.wt.bytes);
    HIP_TRY(hipMemcpyAsync(d, h, l.h_total, hipMemcpyHostToDevice, r->stream));
    if ((rc = f.def.mark(r->stream))) return rc;
    PoseBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.seg = reinterpret_cast<const PoseSegment*>(d + l.seg.off); a.nseg = c.n; a.total = (uint32_t)total;
    a.skins = skins; a.skins_dq = skins_dq; a.morphs = any_morph ? 1u : 0u;
    if (palette && c.on_device) { a.check_palette = palette; a.check_cols = c.per_mesh ? c.check_cols : 4u * c.njoints; }
    if (weights && c.on_device) { a.check_weights = weights; a.check_nweights = c.per_mesh ? c.check_nweights : c.ntargets; }
    a.morphed = any_skin && any_morph ? f.morphed.as<float4>() : nullptr;
    a.skinned = f.skinned.as<float4>();
    a.scratch_len = (uint32_t)std::min<size_t>(std::min(f.skinned.bytes, a.morphed ? f.morphed.bytes : f.skinned.bytes) / 16, 0xFFFFFFFFu);
    a.out_pos = const_cast<float4*>(f.d_pos);
    a.block = c.recompute ? reinterpret_cast<float4*>(d + l.d_nrm.off) : nullptr;
    a.pool_normals = const_cast<float4*>(r->pools.d_normals);
    a.cap_verts = cap_verts; a.cap_indices = cap_indices;
    a.reject = f.d_reject;
    a.rec = reinterpret_cast<const DeformInstance*>(d + l.rec.off); a.rec_seg = reinterpret_cast<const uint32_t*>(d + l.rec_seg.off);
    a.nrec = (uint32_t)rec.size(); a.work = (uint32_t)work;
    a.slot_of = f.d_slot_of;
    if (c.per_mesh) { a.inst_m = f.xf.m.as<const float4>(); a.num_inst = (uint32_t)f.inst.size(); }
    HIP_TRY(launch_pose_batch(r->sv, a, r->stream));
    changed = work != 0;      // no instance of any mesh of the batch: no triangle changes
    return FRT_OK;
}
// A posing call behind its checks, in its call frame: the batch, then (a triangle was written) the scene extent and the refit. Without a palette there
// is no skin launch, without weights no morph launch.
static int pose_meshes(frt_renderer* r, const char* call, uint32_t n, const uint32_t* mesh_ids, const float* palette, uint32_t njoints, const float* weights, uint32_t ntargets, uint32_t flags) {
    PoseBatchCall c;
    c.call = call; c.n = n; c.mesh_ids = mesh_ids; c.on_device = (flags & FRT_DEFORM_DEVICE) != 0; c.recompute = (flags & FRT_DEFORM_RECOMPUTE_NORMALS) != 0;
    c.palette = palette; c.njoints = njoints;
    c.weights = weights; c.ntargets = ntargets;
    return edit_frame(r, true, [&]() -> int {
        bool changed = false;
        if (const int rc = pose_meshes_body(r, c, changed)) return rc;
        return changed ? refit_scene(r) : FRT_OK;
    });
}
// The entry and the flags, the batch itself and every mesh as its single call checks it (check_posed_meshes), then the device pointers.
int frt_renderer_set_mesh_poses(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (const int rc = check_entry(r, "set_mesh_poses", kEditChecks | kRefit)) return rc;
    if (flags & ~kDeformFlags) return fail(FRT_ERR_INVALID_ARG, "set_mesh_poses: unknown flag bits");
    const bool dev = (flags & FRT_DEFORM_DEVICE) != 0, skin = joint_mats || njoints, morph = morph_weights || ntargets;
    const std::string bad = check_posed_meshes(r, n, mesh_ids, skin, joint_mats, njoints, morph, morph_weights, ntargets, !dev);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_poses: " + bad);
    if (dev && skin) if (const int rc = check_device_input(r, joint_mats, (size_t)njoints * 64, 16, "set_mesh_poses", "joint matrices")) return rc;
    if (dev && morph) if (const int rc = check_device_input(r, morph_weights, (size_t)ntargets * 4, 4, "set_mesh_poses", "morph weights")) return rc;
    return pose_meshes(r, "set_mesh_poses", n, mesh_ids, joint_mats, njoints, morph_weights, ntargets, flags);
}
// The three single-mesh calls keep their own checks, in their own order and under their own names, and then pose a batch of one mesh.
int frt_renderer_set_mesh_morph_weights(frt_renderer* r, uint32_t mesh_id, const float* weights, uint32_t ntargets, uint32_t flags) {
    if (const int rc = check_mesh_call(r, "set_mesh_morph_weights", mesh_id, flags, kDeformFlags)) return rc;
    if (const int rc = check_morph_input(r, "set_mesh_morph_weights", mesh_id, weights, ntargets, (flags & FRT_DEFORM_DEVICE) != 0)) return rc;
    return pose_meshes(r, "set_mesh_morph_weights", 1u, &mesh_id, nullptr, 0u, weights, ntargets, flags);
}
// The pose's checks, the palette's device pointer, then (with morph weights or a target count) the morph's; the palette's finiteness is the skin launch's
// to check when it is device memory.
int frt_renderer_set_mesh_pose_ex(frt_renderer* r, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, const float* morph_weights, uint32_t ntargets, uint32_t flags) {
    if (const int rc = check_mesh_call(r, "set_mesh_pose", mesh_id, flags, kDeformFlags)) return rc;
    const bool dev = (flags & FRT_DEFORM_DEVICE) != 0, morph = morph_weights || ntargets;
    const std::string bad = check_mesh_pose(joint_mats, njoints, mesh_id < r->rf.skins.size() ? r->rf.skins[mesh_id].count : 0u, !dev);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_mesh_pose: " + bad);
    if (dev) if (const int rc = check_device_input(r, joint_mats, (size_t)njoints * 64, 16, "set_mesh_pose", "joint matrices")) return rc;
    if (morph) if (const int rc = check_morph_input(r, "set_mesh_pose", mesh_id, morph_weights, ntargets, dev)) return rc;
    return pose_meshes(r, "set_mesh_pose", 1u, &mesh_id, joint_mats, njoints, morph_weights, ntargets, flags);
}
int frt_renderer_set_mesh_pose(frt_renderer* r, uint32_t mesh_id, const float* joint_mats, uint32_t njoints, uint32_t flags) {
    return frt_renderer_set_mesh_pose_ex(r, mesh_id, joint_mats, njoints, nullptr, 0u, flags);
}

} // extern "C"
// check_device_input for the other files of the library (frt_renderer_state.hpp).
int frt::check_device_block(const frt_renderer* r, const void* p, size_t bytes, size_t align, const char* call, const char* what, const char* flag) { return check_device_input(r, p, bytes, align, call, what, flag); }
// frt_renderer_animate_cast (frt_animation.hip; DESIGN.md §11, "Animating a cast") behind its checks and its rig launch: one call frame, so the
// speculation is dropped once; the matrix table current; the instance half as one device-input transform; the mesh half as one pose batch that reads
// the table (the mirror, stale from the first half on, is not read back: no wait for the stream); then, if either wrote a triangle, one scene extent
// and one refit. The halves reject on their own, each through its own flag and counter.
int frt::apply_cast(frt_renderer* r, const CastApply& c) {
    return edit_frame(r, true, [&]() -> int {
        if (const int rc = ensure_transform_tables(r)) return rc;
        bool moved = false, posed = false;
        if (c.ninst) {
            if (const int rc = transform_instances_device(r, c.ninst, c.ids, c.mats)) return rc;
            moved = true;
        }
        if (!c.meshes.empty()) {
            PoseBatchCall p;
            p.call = "animate_cast"; p.n = (uint32_t)c.meshes.size(); p.per_mesh = c.meshes.data(); p.on_device = true; p.recompute = c.recompute;
            p.palette = c.palettes; p.check_cols = c.cols; p.weights = c.weights; p.check_nweights = c.nweights;
            if (const int rc = pose_meshes_body(r, p, posed)) return rc;
        }
        return moved || posed ? refit_scene(r) : FRT_OK;
    });
}
extern "C" {

// ------------------------------------------------------------------------------------------------ materials, lights, textures
// The speculation is dropped: its G-buffer and T-trace have read the materials. All four calls stage through r->look: what a call uploads is written
// into the pinned block and copied from there, on the main stream, into the replica's tables (or, for the instance records of set_instance_materials,
// into the device block its one kernel reads).
int frt_renderer_set_materials(frt_renderer* r, uint32_t n, const uint32_t* ids, const frt_material* mats) {
    if (const int rc = check_entry(r, "set_materials", kLookChecks)) return rc;
    const std::string bad = check_set_materials(n, ids, mats, r->sv.num_materials, r->rf.color_layers, r->rf.data_layers, r->sv.num_lights);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_materials: " + bad);
    if (n == 0) return FRT_OK;
    return edit_frame(r, true, [&]() -> int {
        // ascending ids, of an id given twice its last value: no two copies overlap, and a run of consecutive ids is one copy
        std::vector<std::pair<uint32_t, uint32_t>> e(n);
        for (uint32_t k = 0; k < n; ++k) e[k] = {ids[k], k};
        std::sort(e.begin(), e.end());
        size_t m = 0;
        for (size_t k = 0; k < e.size(); ++k) if (k + 1 == e.size() || e[k + 1].first != e[k].first) e[m++] = e[k];
        e.resize(m);
        if (const int rc = r->look.reserve(m * sizeof(frt_material), 0, r->stream)) return rc;
        for (size_t k = 0; k < m; ++k) memcpy(r->look.h + k * sizeof(frt_material), mats + e[k].second, sizeof(frt_material));
        for (size_t k = 0; k < m;) {
            size_t run = 1;
            while (k + run < m && e[k + run].first == e[k].first + (uint32_t)run) ++run;
            HIP_TRY(hipMemcpyAsync(const_cast<MaterialView*>(r->sv.materials) + e[k].first, r->look.h + k * sizeof(frt_material), run * sizeof(frt_material), hipMemcpyHostToDevice, r->stream));
            k += run;
        }
        return r->look.mark(r->stream);
    });
}

int frt_renderer_set_instance_materials(frt_renderer* r, uint32_t n, const uint32_t* iids, const uint32_t* mids) {
    if (const int rc = check_entry(r, "set_instance_materials", kLookChecks)) return rc;
    const std::string bad = check_set_instance_materials(n, iids, mids, r->rf.inst, r->sv.num_materials);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_instance_materials: " + bad);
    if (n == 0) return FRT_OK;
    return edit_frame(r, true, [&]() -> int {
        RefitState& f = r->rf;
        drop_transform_tables(r, false);
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
        if (const int rc = r->look.upload(rec.data(), rec.size() * sizeof(MaterialEditInstance), r->stream)) return rc;
        const MaterialEditArgs a{reinterpret_cast<const MaterialEditInstance*>(r->look.d), (uint32_t)rec.size(), work, (uint32_t)f.inst.size()};
        HIP_TRY(launch_instance_materials(r->sv, a, r->stream));
        return FRT_OK;
    });
}

int frt_renderer_set_light_emission(frt_renderer* r, uint32_t light, const float color[3], float intensity) {
    if (const int rc = check_entry(r, "set_light_emission", kLookChecks)) return rc;
    if (!color) return fail(FRT_ERR_INVALID_ARG, "set_light_emission: null colour");
    if (light >= r->sv.num_lights) return fail(FRT_ERR_INVALID_ARG, "set_light_emission: light " + std::to_string(light) + " out of range (" + std::to_string(r->sv.num_lights) + " lights)");
    return edit_frame(r, true, [&]() -> int {
        RefitState& f = r->rf;
        float up[8] = {color[0], color[1], color[2], intensity, 0.0f, 0.0f, 0.0f, 0.0f};      // [emission | emissive_factor]
        light_emissive_factor(color, intensity, up + 4);
        memcpy(f.lights[light].emission, up, 16);      // the mirror a later set_instance_transforms re-creates a moved light's record from
        drop_transform_tables(r, false);
        if (const int rc = r->look.reserve(sizeof(up), 0, r->stream)) return rc;
        memcpy(r->look.h, up, sizeof(up));
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(const_cast<LightView*>(r->sv.lights) + light) + offsetof(LightView, emission), r->look.h, 16, hipMemcpyHostToDevice, r->stream));
        const int i = light_instance(f.inst, light);
        if (i >= 0 && f.inst[(size_t)i].mat_id < r->sv.num_materials)
            HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(const_cast<MaterialView*>(r->sv.materials) + f.inst[(size_t)i].mat_id) + offsetof(MaterialView, emissive_factor), r->look.h + 16, 12, hipMemcpyHostToDevice, r->stream));
        return r->look.mark(r->stream);
    });
}

int frt_renderer_set_texture(frt_renderer* r, int kind, uint32_t layer, const uint8_t* rgba8) {
    if (const int rc = check_entry(r, "set_texture", kLookChecks)) return rc;
    const std::string bad = check_set_texture(kind, layer, rgba8, r->rf.color_layers, r->rf.data_layers);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_texture: " + bad);
    return edit_frame(r, true, [&]() -> int {
        if (const int rc = r->look.reserve(kTextureLayerBytes, 0, r->stream)) return rc;
        memcpy(r->look.h, rgba8, kTextureLayerBytes);
        uint8_t* dst = const_cast<uint8_t*>(kind == 0 ? r->sv.color_tex : r->sv.data_tex) + (size_t)layer * kTextureLayerBytes;
        HIP_TRY(hipMemcpyAsync(dst, r->look.h, kTextureLayerBytes, hipMemcpyHostToDevice, r->stream));
        return r->look.mark(r->stream);
    });
}

// ------------------------------------------------------------------------------------------------ tree rebuild ("Rebuild")
// A speculated frame that ran ahead on the old tree is kept: both trees give the same hits. The call waits for the main stream, so when it returns no
// kernel reads the buffers that left the replica; they stay allocated and are what the next rebuild builds into.

// The buffers a rebuild builds into, with room for a tree over the triangle capacity: the scratch, the spare triangle slots and id -> slot table, and
// the quad-node buffer that is not in use (the host-built tree's buffer may be smaller than a device tree needs, so it is never built into; the second
// buffer is allocated by the second rebuild). None of them is part of the replica, and no kernel of an earlier call still uses them (every rebuild
// waits for its stream).
static int rebuild_prepare(frt_renderer* r, uint32_t num_tris, uint32_t mode, RebuildTarget& target) {
    RebuildState& b = r->rbt;
    const uint32_t cap = std::max(pool_cap(r, kPoolTris), num_tris);
    HIP_TRY(rebuild_reserve(b.scratch, cap));
    if (mode == FRT_REBUILD_SAH && num_tris > 2u) HIP_TRY(ploc_reserve(b.scratch, cap));      // the refined mode's own scratch, at its first call (and after a growth) only
    OwnedBuf& nodes = b.nodes[r->sv.nodes4 == b.nodes[0].p ? 1 : 0];
    int rc;
    if ((rc = b.tris.ensure(r, (size_t)cap * sizeof(TriSlot)))) return rc;
    if ((rc = b.slot_of.ensure(r, (size_t)cap * sizeof(uint32_t)))) return rc;
    if ((rc = nodes.ensure(r, (size_t)rebuild_max_nodes(cap) * sizeof(QuadNode)))) return rc;
    target = RebuildTarget{b.tris.as<float4>(), nodes.as<float4>(), b.slot_of.as<uint32_t>()};
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
// The finished tree enters the replica; the slots and the table that leave it are what the next rebuild builds into.
static void rebuild_swap(frt_renderer* r, const RebuildTarget& target, const RebuildResult& res) {
    RebuildState& b = r->rbt;
    SceneView& sv = r->sv;
    const size_t cap = pool_cap(r, kPoolTris);
    b.tris.trade(sv.tris, cap * sizeof(TriSlot)); b.slot_of.trade(r->rf.d_slot_of, cap * sizeof(uint32_t));
    sv.nodes4 = target.nodes; sv.num_nodes4 = res.num_nodes;
    r->rf.quad_levels = res.levels;
    r->rf.pair_levels.assign(1, 0u);       // later refits skip the pair levels
    r->rf.ok = true;
    r->wg_rows = res.stack_need + 1u;
    r->vote = walk_votes(res.num_nodes);
    b.done = true; b.origin = res.origin;
}
int frt_renderer_rebuild_tree(frt_renderer* r) { return frt_renderer_rebuild_tree_ex(r, FRT_REBUILD_MORTON); }
int frt_renderer_rebuild_tree_ex(frt_renderer* r, uint32_t mode) {
    if (const int rc = check_entry(r, "rebuild_tree", kEditChecks)) return rc;
    if (mode != FRT_REBUILD_MORTON && mode != FRT_REBUILD_SAH) return fail(FRT_ERR_INVALID_ARG, "rebuild_tree: unknown mode (FRT_REBUILD_MORTON, FRT_REBUILD_SAH)");
    return edit_frame(r, false, [&]() -> int {
        RebuildTarget target;
        RebuildResult res;
        if (const int rc = rebuild_into(r, r->sv, r->rf.d_slot_of, mode, "rebuild_tree", target, res)) return rc;
        rebuild_swap(r, target, res);
        return FRT_OK;
    });
}

// ------------------------------------------------------------------------------------------------ adding and removing instances
// The speculation is dropped: it was traced on the old geometry. The kernels of frt_instance_edit.hip write buffers that are not part of the replica
// (InstanceEditState); the scene-extent pass and the rebuild follow them on the main stream and read only those; the rebuild waits for the stream, and
// only then — the tree is known to fit the traversal stack — do the new triangles, shading records, instance records, id -> slot table and tree enter
// the replica in one step, with the host bookkeeping (RefitState::inst). A call that is refused or fails before that step leaves the replica as it was
// (the extent word is made again from the replica's triangles).

// Room for `need_tris` triangles and `need_inst` instances in the replica's buffers sized by them (from the first such call on they have a capacity
// apart from their count) and in the edit's own; the rebuild's buffers follow in rebuild_prepare.
static int reserve_edit(frt_renderer* r, uint32_t need_tris, uint32_t need_inst) {
    InstanceEditState& e = r->ie;
    pin_capacity(r, kPoolTris); pin_capacity(r, kPoolInstances);
    uint32_t need[kPoolCount] = {};
    need[kPoolTris] = need_tris; need[kPoolInstances] = need_inst;
    int rc;
    if ((rc = reserve_pools(r, need))) return rc;
    const size_t tris = pool_cap(r, kPoolTris), inst = pool_cap(r, kPoolInstances);
    if ((rc = e.tris.ensure(r, tris * sizeof(TriSlot)))) return rc;
    if ((rc = e.shade_tris.ensure(r, tris * sizeof(ShadeTri)))) return rc;
    if ((rc = e.slot_of.ensure(r, tris * sizeof(uint32_t)))) return rc;
    return e.instances.ensure(r, inst * sizeof(InstanceView));
}
static InstanceEditTarget edit_target(const InstanceEditState& e) {
    return InstanceEditTarget{e.tris.as<float4>(), e.slot_of.as<uint32_t>(), e.shade_tris.as<float4>(), e.instances.as<InstanceView>()};
}
// What both calls end with: the extent and the tree of the triangles the edit wrote, then everything enters the replica together.
static int commit_instance_edit(frt_renderer* r, uint32_t num_tris, std::vector<InstanceRec>& inst, uint32_t mode, const char* what) {
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    unsigned int* ext = const_cast<unsigned int*>(r->rf.d_ext);
    SceneView nv = sv;
    nv.tris = e.tris.as<float4>(); nv.shade_tris = e.shade_tris.as<float4>(); nv.instances = e.instances.as<InstanceView>(); nv.num_tris = num_tris;
    HIP_TRY(launch_scene_extent(nv, ext, r->stream));
    RebuildTarget target;
    RebuildResult res;
    const int rc = rebuild_into(r, nv, e.slot_of.as<uint32_t>(), mode, what, target, res);
    if (rc) {
        if (rc != FRT_ERR_HIP) {      // refused: the extent word of the replica's own triangles again (fail()'s message is kept)
            HIP_TRY(launch_scene_extent(sv, ext, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
        }
        return rc;
    }
    rebuild_swap(r, target, res);      // (what left the replica there are the spare slots and table of the next rebuild)
    e.shade_tris.trade(sv.shade_tris, (size_t)pool_cap(r, kPoolTris) * sizeof(ShadeTri));
    e.instances.trade(sv.instances, (size_t)pool_cap(r, kPoolInstances) * sizeof(InstanceView));
    sv.num_tris = num_tris;
    r->rf.inst.swap(inst);
    return FRT_OK;
}

// `n` > 0 checked instances join the replica; returns the id of the first. The caller has opened the frame.
// (`light` >= 0, register_*_light of §15: the first new instance carries the link to that light, of kind `light_kind`)
static int add_instances(frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, const uint32_t* mat_ids, const float* mats, uint32_t mode, int32_t light = -1, uint32_t light_kind = 0) {
    RefitState& f = r->rf;
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    const uint32_t old_tris = sv.num_tris, old_inst = (uint32_t)f.inst.size();
    if (const int rc0 = sync_matrix_mirror(r)) return rc0;      // (the old instances' records are copied below, matrices included)
    drop_transform_tables(r, true);
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
    int rc;
    if ((rc = reserve_edit(r, num_tris, num_inst))) return rc;
    if ((rc = ensure_normals(r))) return rc;
    if ((rc = e.rec.upload(rec.data(), rec.size() * sizeof(AppendInstance), r->stream))) return rc;
    // what stays: the old slots where they are (and their table), the old shading and instance records
    const InstanceEditTarget out = edit_target(e);
    HIP_TRY(hipMemcpyAsync(out.tris, sv.tris, (size_t)old_tris * sizeof(TriSlot), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(out.slot_of, f.d_slot_of, (size_t)old_tris * sizeof(uint32_t), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(out.shade_tris, sv.shade_tris, (size_t)old_tris * sizeof(ShadeTri), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(out.instances, sv.instances, (size_t)old_inst * sizeof(InstanceView), hipMemcpyDeviceToDevice, r->stream));
    const AppendArgs a{reinterpret_cast<const AppendInstance*>(e.rec.d), n, work, f.d_pos, r->pools.d_normals, num_tris, num_inst, out};
    HIP_TRY(launch_instances_append(sv, a, r->stream));
    if ((rc = commit_instance_edit(r, num_tris, inst, mode, "add_instances"))) return rc;
    return (int)old_inst;
}

// The instances `gone` (checked, ascending, not empty) leave the replica. The caller has opened the frame.
static int remove_instances(frt_renderer* r, const std::vector<uint32_t>& gone, uint32_t mode) {
    RefitState& f = r->rf;
    InstanceEditState& e = r->ie;
    SceneView& sv = r->sv;
    const uint32_t old_tris = sv.num_tris, old_inst = (uint32_t)f.inst.size();
    if (const int rc0 = sync_matrix_mirror(r)) return rc0;      // (the survivors' records are copied below, matrices included)
    drop_transform_tables(r, true);
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
    int rc;
    if ((rc = reserve_edit(r, num_tris, num_inst))) return rc;
    if ((rc = e.rec.upload(rng.data(), rng.size() * sizeof(RemovedRange), r->stream))) return rc;
    const RemoveArgs a{reinterpret_cast<const RemovedRange*>(e.rec.d), (uint32_t)rng.size(), f.d_slot_of, old_tris, old_inst, num_tris, num_inst, edit_target(e)};
    HIP_TRY(launch_instances_remove(sv, a, r->stream));
    if ((rc = commit_instance_edit(r, num_tris, inst, mode, "remove_instances"))) return rc;
    // an instance rig binding follows its instances to their new ids (the next animate_instances uploads them); one that names an instance that left is unbound
    const std::vector<uint32_t> map = removal_map(old_inst, gone);
    for (RigBinding& b : r->rigs) {
        if (!b.live || b.kind != kRigInstances) continue;
        bool lost = false;
        for (uint32_t& i : b.instance_ids) { if (i >= old_inst || map[i] == kGone) lost = true; else i = map[i]; }
        if (lost) { b.release(r); b = RigBinding(); } else b.ids_stale = true;
    }
    return FRT_OK;
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
    return edit_frame(r, true, [&]() -> int { return add_instances(r, n, mesh_ids, mat_ids, m_colmajor16, rebuild_mode); });
}
int frt_renderer_remove_instances(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode) {
    if (const int rc = check_entry(r, "remove_instances", kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode("remove_instances", rebuild_mode)) return rc;
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_instances(n, ids, r->rf.inst, gone, why)) return fail(rc, "remove_instances: " + why);
    if (gone.empty()) return FRT_OK;
    return edit_frame(r, true, [&]() -> int { return remove_instances(r, gone, rebuild_mode); });
}

// ------------------------------------------------------------------------------------------------ new meshes, materials, layers, lights
// What a call uploads is written into the pinned block of r->pools.up and copied from there, on the main stream: materials, lights and texture layers
// straight into the replica's pools, the vertices and indices of new meshes into the device block mesh_append_kernel reads. A pool that is too small
// grows first (reserve_pools). The host bookkeeping (RefitState) and the counts of the SceneView follow when everything is enqueued, so that the
// edits of §11 - §14 accept the new ids.

// `bytes` from `src` through the pinned block at `h_off` to `dst`, on the main stream (the caller has reserved the block and marks it afterwards).
static int staged_copy(frt_renderer* r, size_t h_off, const void* src, void* dst, size_t bytes) {
    memcpy(r->pools.up.h + h_off, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, r->pools.up.h + h_off, bytes, hipMemcpyHostToDevice, r->stream));
    return FRT_OK;
}
// `n` records of `bytes_each` join the pool `p` behind its `old` ones (`live_ptr`: the replica's pointer to the pool's buffer, read once the pool has its room).
static int append_records(frt_renderer* r, int p, uint32_t old, uint32_t n, const void* src, size_t bytes_each, const void* live_ptr) {
    uint32_t need[kPoolCount] = {};
    need[p] = old + n;
    int rc;
    if ((rc = reserve_pools(r, need))) return rc;
    const size_t bytes = (size_t)n * bytes_each;
    if ((rc = r->pools.up.reserve(bytes, 0, r->stream))) return rc;
    uint8_t* live = static_cast<uint8_t*>(const_cast<void*>(*static_cast<const void* const*>(live_ptr)));
    if ((rc = staged_copy(r, 0, src, live + (size_t)old * bytes_each, bytes))) return rc;
    return r->pools.up.mark(r->stream);
}

int frt_renderer_add_meshes(frt_renderer* r, uint32_t n, const frt_mesh_data* meshes) {
    if (const int rc = check_entry(r, "add_meshes", kLookChecks)) return rc;
    RefitState& f = r->rf;
    const uint32_t old_meshes = (uint32_t)f.mesh_tris.size(), old_verts = pool_count(r, kPoolVerts), old_indices = pool_count(r, kPoolIndices);
    const uint64_t pos_verts = f.pos_offset.empty() ? 0u : (uint64_t)f.pos_offset.back() + f.vert_count.back();
    if (pos_verts != old_verts) return fail(FRT_ERR_STATE, "add_meshes: the replica's positions and attributes are not numbered alike");
    std::string why;
    if (const int rc = check_add_meshes(n, meshes, old_verts, old_indices, why)) return fail(rc, "add_meshes: " + why);
    if (n == 0) return (int)old_meshes;
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; ++k) total += (uint64_t)meshes[k].nverts + meshes[k].nidx;
    if (total > 0xFFFFFF00ull || (uint64_t)old_meshes + n > 0x7FFFFFFFull) return fail(FRT_ERR_LIMIT, "add_meshes: too many vertices and indices, or meshes, in one call");
    return edit_frame(r, true, [&]() -> int {
        Staging& up = r->pools.up;
        drop_transform_tables(r, false);
        std::vector<MeshAppend> rec;
        uint32_t nv = 0, ni = 0;
        pack_mesh_appends(n, meshes, old_verts, old_indices, rec, nv, ni);
        int rc;
        if ((rc = ensure_normals(r))) return rc;      // (at the replica's present size; the pool of the vertices grows with the others below)
        uint32_t need[kPoolCount] = {};
        need[kPoolVerts] = old_verts + nv; need[kPoolIndices] = old_indices + ni; need[kPoolMeshes] = old_meshes + n;
        if ((rc = reserve_pools(r, need))) return rc;
        // one block: [records | positions | attributes | indices], each part 16-byte aligned (32 n, 16 nv and 32 nv bytes in front of the indices)
        const size_t rec_bytes = (size_t)n * sizeof(MeshAppend), pos_bytes = (size_t)nv * 16, attr_bytes = (size_t)nv * sizeof(frt_vertex_attr), idx_bytes = (size_t)ni * 4;
        const size_t pos_at = rec_bytes, attr_at = pos_at + pos_bytes, idx_at = attr_at + attr_bytes, all_bytes = idx_at + idx_bytes;
        if ((rc = up.reserve(all_bytes, all_bytes, r->stream))) return rc;
        memcpy(up.h, rec.data(), rec_bytes);
        for (uint32_t k = 0; k < n; ++k) {
            memcpy(up.h + pos_at + (size_t)rec[k].vert_begin * 16, meshes[k].pos4, (size_t)meshes[k].nverts * 16);
            memcpy(up.h + attr_at + (size_t)rec[k].vert_begin * sizeof(frt_vertex_attr), meshes[k].attrs, (size_t)meshes[k].nverts * sizeof(frt_vertex_attr));
            memcpy(up.h + idx_at + (size_t)rec[k].index_begin * 4, meshes[k].idx, (size_t)meshes[k].nidx * 4);
        }
        HIP_TRY(hipMemcpyAsync(up.d, up.h, all_bytes, hipMemcpyHostToDevice, r->stream));
        if ((rc = up.mark(r->stream))) return rc;
        MeshAppendArgs a{};
        a.rec = reinterpret_cast<const MeshAppend*>(up.d); a.nrec = n; a.nverts = nv; a.nidx = ni;
        a.pos = reinterpret_cast<const float4*>(up.d + pos_at); a.attrs = reinterpret_cast<const float4*>(up.d + attr_at); a.idx = reinterpret_cast<const uint32_t*>(up.d + idx_at);
        a.out_pos = const_cast<float4*>(f.d_pos); a.out_attrs = reinterpret_cast<float4*>(const_cast<VertexAttrView*>(r->sv.attributes));
        a.out_normals = const_cast<float4*>(r->pools.d_normals); a.out_idx = const_cast<uint32_t*>(r->sv.indices); a.out_infos = const_cast<MeshInfoView*>(r->sv.mesh_infos);
        a.mesh_base = old_meshes;
        a.cap_verts = pool_cap(r, kPoolVerts); a.cap_indices = pool_cap(r, kPoolIndices); a.cap_meshes = pool_cap(r, kPoolMeshes);
        HIP_TRY(launch_mesh_append(a, r->stream));
        for (uint32_t k = 0; k < n; ++k) {
            f.pos_offset.push_back(rec[k].vert_base); f.attr_offset.push_back(rec[k].vert_base); f.index_offset.push_back(rec[k].index_base);
            f.vert_count.push_back(rec[k].nverts); f.mesh_tris.push_back(rec[k].nidx / 3u);
        }
        return (int)old_meshes;
    });
}

int frt_renderer_add_materials(frt_renderer* r, uint32_t n, const frt_material* materials) {
    if (const int rc = check_entry(r, "add_materials", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_materials(n, materials, r->sv.num_materials, r->rf.color_layers, r->rf.data_layers, r->sv.num_lights, why)) return fail(rc, "add_materials: " + why);
    if (n == 0) return (int)r->sv.num_materials;
    return edit_frame(r, true, [&]() -> int {
        const uint32_t old = r->sv.num_materials;
        if (const int rc = append_records(r, kPoolMaterials, old, n, materials, sizeof(frt_material), &r->sv.materials)) return rc;
        r->sv.num_materials = old + n;
        return (int)old;
    });
}

int frt_renderer_add_texture(frt_renderer* r, int kind, const uint8_t* rgba8) {
    if (const int rc = check_entry(r, "add_texture", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_texture(kind, rgba8, r->rf.color_layers, r->rf.data_layers, why)) return fail(rc, "add_texture: " + why);
    return edit_frame(r, true, [&]() -> int {
        uint32_t& layers = kind == 0 ? r->rf.color_layers : r->rf.data_layers;
        if (const int rc = append_records(r, kind == 0 ? kPoolColor : kPoolData, layers, 1u, rgba8, kTextureLayerBytes, kind == 0 ? &r->sv.color_tex : &r->sv.data_tex)) return rc;
        return (int)layers++;
    });
}

int frt_renderer_add_lights(frt_renderer* r, uint32_t n, const frt_light* lights) {
    if (const int rc = check_entry(r, "add_lights", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_add_lights(n, lights, why)) return fail(rc, "add_lights: " + why);
    if ((uint64_t)r->sv.num_lights + n > 0x7FFFFFFFull) return fail(FRT_ERR_LIMIT, "add_lights: a material's light_index is a signed 32-bit number");
    if (n == 0) return (int)r->sv.num_lights;
    return edit_frame(r, true, [&]() -> int {
        const uint32_t old = r->sv.num_lights;
        if (const int rc = append_records(r, kPoolLights, old, n, lights, sizeof(frt_light), &r->sv.lights)) return rc;
        r->rf.lights.insert(r->rf.lights.end(), lights, lights + n);
        r->sv.num_lights = old + n;
        return (int)old;
    });
}

// register_quad_light / register_sphere_light of the builder (frt_scene.cpp) on the replica: the material and the light record are made by the builder's
// own functions; the pools get their room first (a refusal there changes nothing), then the instance joins (add_instances) with the ids the material
// and the light are about to get, and only when its tree is in place do the two records follow and the counts move.
static int register_light(frt_renderer* r, uint32_t mesh_id, const float* m, const float* color, float intensity, uint32_t mode, uint32_t kind, const char* what) {
    if (const int rc = check_entry(r, what, kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode(what, mode)) return rc;
    if (!m || !color) return fail(FRT_ERR_INVALID_ARG, std::string(what) + ": null matrix or colour");
    const uint32_t mat_id = r->sv.num_materials, light_id = r->sv.num_lights;
    std::string why;
    if (mat_id >= kMaxMaterials) return fail(FRT_ERR_LIMIT, std::string(what) + ": more than 65535 materials");
    if (const int rc = check_add_instances(1, &mesh_id, &mat_id, m, r->rf.mesh_tris, (size_t)mat_id + 1u, r->sv.num_tris, why)) return fail(rc, std::string(what) + ": " + why);
    Mat4 t; memcpy(t.m, m, sizeof(t.m));
    const float em[4] = {color[0], color[1], color[2], intensity};
    const frt_light light = kind == 0 ? quad_light_record(t, em) : sphere_light_record(t, em);
    if (const int rc = check_add_lights(1, &light, why)) return fail(rc, std::string(what) + ": the light this transform, colour and intensity make: " + why);
    const frt_material mat = light_emissive_material(light_id, color, intensity);
    return edit_frame(r, true, [&]() -> int {
        uint32_t need[kPoolCount] = {};
        need[kPoolMaterials] = mat_id + 1u; need[kPoolLights] = light_id + 1u;
        int rc;
        if ((rc = reserve_pools(r, need))) return rc;
        if ((rc = r->pools.up.reserve(sizeof(mat) + sizeof(light), 0, r->stream))) return rc;
        if ((rc = add_instances(r, 1, &mesh_id, &mat_id, m, mode, (int32_t)light_id, kind)) < 0) return rc;
        if ((rc = staged_copy(r, 0, &mat, const_cast<MaterialView*>(r->sv.materials) + mat_id, sizeof(mat)))) return rc;
        if ((rc = staged_copy(r, sizeof(mat), &light, const_cast<LightView*>(r->sv.lights) + light_id, sizeof(light)))) return rc;
        if ((rc = r->pools.up.mark(r->stream))) return rc;
        r->rf.lights.push_back(light);
        drop_transform_tables(r, false);      // (the new instance's light record is in the mirror only now)
        r->sv.num_materials = mat_id + 1u; r->sv.num_lights = light_id + 1u;
        return (int)light_id;
    });
}
int frt_renderer_register_quad_light(frt_renderer* r, uint32_t mesh_id, const float m[16], const float color[3], float intensity, uint32_t rebuild_mode) {
    return register_light(r, mesh_id, m, color, intensity, rebuild_mode, 0u, "register_quad_light");
}
int frt_renderer_register_sphere_light(frt_renderer* r, uint32_t mesh_id, const float m[16], const float color[3], float intensity, uint32_t rebuild_mode) {
    return register_light(r, mesh_id, m, color, intensity, rebuild_mode, 1u, "register_sphere_light");
}

// ------------------------------------------------------------------------------------------------ removing meshes, materials, layers, lights
// The speculation is dropped: it has read the ids that change. The tables of a call (old -> new ids, removed spans) are staged through r->rm.tab. A pool
// that closes up is compacted by a kernel into its spare buffer (RemoveState::spare, with room for the pool's capacity), which trades places with the
// replica's on the host once every launch of the call is enqueued; the buffer that left is the next removal's spare, and the next kernel that writes it
// is behind this call's readers on the same stream. Surviving records are renumbered in place, one word per thread, and so is gpos.w of every G-buffer
// set the renderer owns. Nothing waits for the device unless a spare has to be (re)allocated, except the two checks that read the material table back.
static int stage_words(frt_renderer* r, const std::vector<uint32_t>& w, const uint32_t** d) {
    if (const int rc = r->rm.tab.upload(w.data(), w.size() * 4, r->stream)) return rc;
    *d = reinterpret_cast<const uint32_t*>(r->rm.tab.d);
    return FRT_OK;
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
// Runs before the call's frame, under its own rules: it orders nothing and drops nothing.
static int read_materials(frt_renderer* r, std::vector<frt_material>& out) {
    auto read = [&]() -> int {
        FRT_DEVICE(r);
        if (const int rc = sync_all(r)) return rc;
        out.resize(r->sv.num_materials);
        if (!out.empty()) HIP_TRY(hipMemcpy(out.data(), r->sv.materials, out.size() * sizeof(frt_material), hipMemcpyDeviceToHost));
        return FRT_OK;
    };
    const int rc = read();
    if (rc == FRT_ERR_HIP) r->failed = true;
    return rc;
}

// What removing the 64-byte records `gone` (checked, ascending, not empty) from the pool `p` of `old` records begins with: the pool keeps its room, the
// tables [old -> new id of every record | one span per removed id] are staged (`d`; `map` is the first part on the host), and a kernel compacts the
// survivors of `live` into `spare`. The caller renumbers whatever names the ids and then lets `spare` trade places with `live`.
static int compact_records(frt_renderer* r, int p, OwnedBuf& spare, const void* live, uint32_t old, const std::vector<uint32_t>& gone, std::vector<uint32_t>& map, const uint32_t** d) {
    map = removal_map(old, gone);
    std::vector<uint32_t> words = map;
    for (size_t k = 0; k < gone.size(); ++k) { words.push_back(gone[k] - (uint32_t)k); words.push_back((uint32_t)k + 1u); }
    pin_capacity(r, p);
    int rc;
    if ((rc = spare.ensure(r, (size_t)pool_cap(r, p) * 64u))) return rc;
    if ((rc = stage_words(r, words, d))) return rc;
    const RemovedSpan* spans = reinterpret_cast<const RemovedSpan*>(*d + old);
    HIP_TRY(launch_compact_vec4(static_cast<const float4*>(live), spare.as<float4>(), old - (uint32_t)gone.size(), 4u, spans, (uint32_t)gone.size(), r->stream));
    return FRT_OK;
}
static_assert(sizeof(MaterialView) == 64 && sizeof(LightView) == 64, "compact_records moves four vec4 per record");

// The materials `gone` leave the table; instance records, shading records and the per-pixel history follow. The caller has opened the frame.
static int remove_materials(frt_renderer* r, const std::vector<uint32_t>& gone) {
    SceneView& sv = r->sv;
    OwnedBuf& spare = r->rm.spare[kSpareMaterials];
    const uint32_t old = sv.num_materials;
    std::vector<uint32_t> map;
    const uint32_t* d = nullptr;
    int rc;
    if ((rc = compact_records(r, kPoolMaterials, spare, sv.materials, old, gone, map, &d))) return rc;
    HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<float4*>(sv.shade_tris)), sv.num_tris, 32u, 25u, d, old, r->stream));
    HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<InstanceView*>(sv.instances)), (uint32_t)r->rf.inst.size(), 16u, 1u, d, old, r->stream));
    if ((rc = remap_history(r, d, old))) return rc;
    spare.trade(sv.materials, (size_t)pool_cap(r, kPoolMaterials) * sizeof(MaterialView));
    drop_transform_tables(r, false);
    for (InstanceRec& in : r->rf.inst) if (in.mat_id < old && map[in.mat_id] != kGone) in.mat_id = map[in.mat_id];
    sv.num_materials = old - (uint32_t)gone.size();
    return FRT_OK;
}
// The light records `gone` leave the table; light_index of every material and the light link of every instance follow.
static int remove_light_records(frt_renderer* r, const std::vector<uint32_t>& gone) {
    SceneView& sv = r->sv;
    OwnedBuf& spare = r->rm.spare[kSpareLights];
    const uint32_t old = sv.num_lights;
    std::vector<uint32_t> map;
    const uint32_t* d = nullptr;
    if (const int rc = compact_records(r, kPoolLights, spare, sv.lights, old, gone, map, &d)) return rc;
    HIP_TRY(launch_remap_materials(const_cast<MaterialView*>(sv.materials), sv.num_materials, d, old, kGone, kGone, r->stream));
    spare.trade(sv.lights, (size_t)pool_cap(r, kPoolLights) * sizeof(LightView));
    remove_elements(r->rf.lights, gone);
    drop_transform_tables(r, false);
    for (InstanceRec& in : r->rf.inst) if (in.light >= 0 && (uint32_t)in.light < old && map[(size_t)in.light] != kGone) in.light = (int32_t)map[(size_t)in.light];
    sv.num_lights = old - (uint32_t)gone.size();
    return FRT_OK;
}

int frt_renderer_remove_materials(frt_renderer* r, uint32_t n, const uint32_t* ids) {
    if (const int rc = check_entry(r, "remove_materials", kLookChecks)) return rc;
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_materials(n, ids, r->sv.num_materials, r->rf.inst, gone, why)) return fail(rc, "remove_materials: " + why);
    if (gone.empty()) return FRT_OK;
    return edit_frame(r, true, [&]() -> int { return remove_materials(r, gone); });
}

int frt_renderer_remove_meshes(frt_renderer* r, uint32_t n, const uint32_t* ids) {
    if (const int rc = check_entry(r, "remove_meshes", kLookChecks)) return rc;
    RefitState& f = r->rf;
    if (f.pos_offset != f.attr_offset) return fail(FRT_ERR_STATE, "remove_meshes: the replica's positions and attributes are not numbered alike");
    std::vector<uint32_t> gone;
    std::string why;
    if (const int rc = check_remove_meshes(n, ids, f.mesh_tris.size(), f.inst, gone, why)) return fail(rc, "remove_meshes: " + why);
    if (gone.empty()) return FRT_OK;
    const uint32_t old_meshes = (uint32_t)f.mesh_tris.size(), old_verts = pool_count(r, kPoolVerts), old_indices = pool_count(r, kPoolIndices);
    if (2ull * old_verts > 0xFFFFFF00ull || old_indices > 0xFFFFFF00u) return fail(FRT_ERR_LIMIT, "remove_meshes: too many vertices or indices for one compaction launch");
    return edit_frame(r, true, [&]() -> int {
        SceneView& sv = r->sv;
        OwnedBuf* spare = r->rm.spare;
        const float4*& normals = r->pools.d_normals;
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
        const size_t pos_bytes = (size_t)pool_cap(r, kPoolVerts) * sizeof(float4), attr_bytes = (size_t)pool_cap(r, kPoolVerts) * sizeof(VertexAttrView);
        const size_t idx_bytes = (size_t)pool_cap(r, kPoolIndices) * sizeof(uint32_t), info_bytes = (size_t)pool_cap(r, kPoolMeshes) * sizeof(MeshInfoView);
        int rc;
        if ((rc = spare[kSparePos].ensure(r, pos_bytes))) return rc;
        if ((rc = spare[kSpareAttrs].ensure(r, attr_bytes))) return rc;
        if (normals && (rc = spare[kSpareNormals].ensure(r, pos_bytes))) return rc;
        if ((rc = spare[kSpareIndices].ensure(r, idx_bytes))) return rc;
        if ((rc = spare[kSpareMeshInfos].ensure(r, info_bytes))) return rc;
        const uint32_t* d = nullptr;
        if ((rc = stage_words(r, words, &d))) return rc;
        const RemovedSpan *dm = reinterpret_cast<const RemovedSpan*>(d), *dv = dm + ns, *di = dv + ns;
        HIP_TRY(launch_compact_vec4(f.d_pos, spare[kSparePos].as<float4>(), verts, 1u, dv, ns, r->stream));
        HIP_TRY(launch_compact_vec4(reinterpret_cast<const float4*>(sv.attributes), spare[kSpareAttrs].as<float4>(), verts, 2u, dv, ns, r->stream));
        if (normals) HIP_TRY(launch_compact_vec4(normals, spare[kSpareNormals].as<float4>(), verts, 1u, dv, ns, r->stream));
        HIP_TRY(launch_compact_u32(sv.indices, spare[kSpareIndices].as<uint32_t>(), indices, di, ns, r->stream));
        HIP_TRY(launch_compact_mesh_infos(sv.mesh_infos, spare[kSpareMeshInfos].as<MeshInfoView>(), meshes, dm, dv, di, ns, r->stream));
        HIP_TRY(launch_remap_words(reinterpret_cast<uint32_t*>(const_cast<InstanceView*>(sv.instances)), (uint32_t)f.inst.size(), 16u, 0u, d + 6u * ns, old_meshes, r->stream));
        // everything is enqueued: the new pools enter the replica together, with the host bookkeeping
        spare[kSparePos].trade(f.d_pos, pos_bytes);
        spare[kSpareAttrs].trade(sv.attributes, attr_bytes);
        if (normals) spare[kSpareNormals].trade(normals, pos_bytes);
        spare[kSpareIndices].trade(sv.indices, idx_bytes);
        spare[kSpareMeshInfos].trade(sv.mesh_infos, info_bytes);
        std::vector<uint32_t> vo, io, vc, mt;
        uint32_t v = 0, i = 0;
        for (uint32_t m = 0; m < old_meshes; ++m) {      // the offsets a scratch build gives the survivors
            if (map[m] == kGone) continue;
            vo.push_back(v); io.push_back(i); vc.push_back(f.vert_count[m]); mt.push_back(f.mesh_tris[m]);
            v += f.vert_count[m]; i += index_count[m];
        }
        f.pos_offset = vo; f.attr_offset.swap(vo); f.index_offset.swap(io); f.vert_count.swap(vc); f.mesh_tris.swap(mt);
        // the adjacency of a mesh that leaves is freed (behind a wait: a deformation's kernel may still read it), the survivors' follow their new ids
        f.adj.resize(old_meshes, nullptr);
        bool waited = false;
        for (uint32_t g : gone) {
            if (!f.adj[g]) continue;
            if (!waited) { HIP_TRY(hipStreamSynchronize(r->stream)); waited = true; }
            scene_free(r, f.adj[g]);
        }
        remove_elements(f.adj, gone);
        // and so do the skins and the morph targets
        for (std::vector<RefitState::MeshBinding>* list : {&f.skins, &f.morphs}) {
            if (list->empty()) continue;
            list->resize(old_meshes);
            for (uint32_t g : gone) if ((rc = drop_binding(r, *list, g))) return rc;
            remove_elements(*list, gone);
        }
        // a rig binding follows its meshes to their new ids; one that names a mesh that left is unbound (animate then refuses its number)
        for (RigBinding& b : r->rigs) {
            if (!b.live) continue;
            bool lost = false;
            for (uint32_t& m : b.mesh_ids) { if (m >= old_meshes || map[m] == kGone) lost = true; else m = map[m]; }
            if (lost) { b.rig.release(r); b.palette.release(r); b.weights.release(r); b = RigBinding(); }
        }
        drop_transform_tables(r, false);
        for (InstanceRec& in : f.inst) in.mesh_id = map[in.mesh_id];
        return FRT_OK;
    });
}

// A registered light leaves as the composite register_*_light made: its instance first (remove_instances: the one step that can be refused, by the
// tree; nothing has changed then), then its material, then the record.
int frt_renderer_remove_lights(frt_renderer* r, uint32_t n, const uint32_t* ids, uint32_t rebuild_mode) {
    if (const int rc = check_entry(r, "remove_lights", kEditChecks)) return rc;
    if (const int rc = check_rebuild_mode("remove_lights", rebuild_mode)) return rc;
    if (n == 0) return FRT_OK;
    std::vector<frt_material> mats;
    if (const int rc = read_materials(r, mats)) return rc;
    LightRemoval rem;
    std::string why;
    if (const int rc = check_remove_lights(n, ids, r->sv.num_lights, mats.data(), mats.size(), r->rf.inst, rem, why)) return fail(rc, "remove_lights: " + why);
    if (rem.lights.empty()) return FRT_OK;
    return edit_frame(r, true, [&]() -> int {
        int rc;
        if (!rem.instances.empty() && (rc = remove_instances(r, rem.instances, rebuild_mode))) return rc;
        if (!rem.materials.empty() && (rc = remove_materials(r, rem.materials))) return rc;      // (from here on only a HIP call can fail: the renderer is then failed)
        return remove_light_records(r, rem.lights);
    });
}

// The layers above the removed one move down, one device-to-device copy each in ascending order (source and destination of a copy are different layers;
// a copy's destination is the source of the copy before it, which the stream has finished by then).
int frt_renderer_remove_texture(frt_renderer* r, int kind, uint32_t layer) {
    if (const int rc = check_entry(r, "remove_texture", kLookChecks)) return rc;
    std::string why;
    if (const int rc = check_remove_texture(kind, layer, r->rf.color_layers, r->rf.data_layers, nullptr, 0, why)) return fail(rc, "remove_texture: " + why);      // (what needs no device first)
    std::vector<frt_material> mats;
    if (const int rc = read_materials(r, mats)) return rc;
    if (const int rc = check_remove_texture(kind, layer, r->rf.color_layers, r->rf.data_layers, mats.data(), mats.size(), why)) return fail(rc, "remove_texture: " + why);
    return edit_frame(r, true, [&]() -> int {
        pin_capacity(r, kind == 0 ? kPoolColor : kPoolData);
        uint32_t& layers = kind == 0 ? r->rf.color_layers : r->rf.data_layers;
        uint8_t* base = const_cast<uint8_t*>(kind == 0 ? r->sv.color_tex : r->sv.data_tex);
        for (uint32_t l = layer; l + 1u < layers; ++l)
            HIP_TRY(hipMemcpyAsync(base + (size_t)l * kTextureLayerBytes, base + (size_t)(l + 1u) * kTextureLayerBytes, kTextureLayerBytes, hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(launch_remap_materials(const_cast<MaterialView*>(r->sv.materials), r->sv.num_materials, nullptr, 0u, kind == 0 ? layer : kGone, kind == 1 ? layer : kGone, r->stream));
        --layers;
        return FRT_OK;
    });
}

} // extern "C"
