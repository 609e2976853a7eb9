// frt_scene_read.hip — the calls that read a renderer's scene replica and change nothing of it (include/frt.h): the ray queries,
// frt_renderer_read_scene, and the statistics and counts. Host code only: the query kernels are in frt_query.hip. The edits are in frt_scene_edit.hip.
#include "frt_renderer_state.hpp"

extern "C" {

// ------------------------------------------------------------------------------------------------ ray queries
// Ordering: a query is enqueued on the main stream and only reads the scene replica. Every writer of the replica is on that stream too: the instance
// update and the deformation (their copies, kernels and refit levels; the ahead stream is fenced into the main stream before them), and the rebuild,
// whose kernels run there and which waits for the stream before it swaps the buffers — so the buffers a rebuild builds into are the ones that left the
// replica at the previous rebuild's wait, behind which no query can read them, and a query enqueued after the swap reads the new ones. The frame's
// own kernels on the other streams read the scene as well and write none of it. Nothing here touches frame state, counters, queues or a speculation:
// a query may run while a frame is open, and a query that fails does not mark the renderer as failed.
enum { kQueryClosest = 0, kQueryAny = 1, kQueryPick = 2 };
static int ray_query(frt_renderer* r, int kind, const frt_camera_uniform* cam, uint32_t n, const void* in, void* out, uint32_t flags, const char* what) {
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
    return ray_query(r, kQueryClosest, nullptr, n, rays, out, flags, "trace_closest");
}
int frt_renderer_trace_any(frt_renderer* r, uint32_t n, const frt_ray* rays, uint8_t* occluded_out, uint32_t flags) {
    return ray_query(r, kQueryAny, nullptr, n, rays, occluded_out, flags, "trace_any");
}
int frt_renderer_pick(frt_renderer* r, const frt_camera_uniform* cam, uint32_t n, const uint32_t* xy, frt_ray_hit* out, uint32_t flags) {
    return ray_query(r, kQueryPick, cam, n, xy, out, flags, "pick");
}

// ------------------------------------------------------------------------------------------------ statistics, counts, the replica's arrays
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
int frt_renderer_scene_counts(frt_renderer* r, uint32_t counts[4]) {
    if (!r || !counts) return fail(FRT_ERR_INVALID_ARG, "renderer scene_counts: null");
    counts[0] = r->sv.num_tris; counts[1] = (uint32_t)r->rf.inst.size(); counts[2] = r->sv.num_materials; counts[3] = r->sv.num_lights;
    return FRT_OK;
}
int frt_renderer_pool_counts(frt_renderer* r, uint32_t counts[6]) {
    if (!r || !counts) return fail(FRT_ERR_INVALID_ARG, "renderer pool_counts: null");
    counts[0] = pool_count(r, kPoolMeshes); counts[1] = pool_count(r, kPoolVerts); counts[2] = pool_count(r, kPoolIndices);
    counts[3] = r->rf.color_layers; counts[4] = r->rf.data_layers; counts[5] = r->pools.growths;
    return FRT_OK;
}
int frt_renderer_deform_rejects(frt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(FRT_ERR_INVALID_ARG, "deform_rejects: null");
    *out = 0u;
    if (!r->rf.d_reject) return FRT_OK;      // no device-input deformation yet
    FRT_DEVICE(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(out, r->rf.d_reject + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FRT_OK;
}
int frt_renderer_transform_rejects(frt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(FRT_ERR_INVALID_ARG, "transform_rejects: null");
    *out = 0u;
    if (!r->rf.xf.d_reject) return FRT_OK;      // no device-input transform call yet
    FRT_DEVICE(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(out, r->rf.xf.d_reject + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FRT_OK;
}
int frt_renderer_read_scene(frt_renderer* r, int which, void* out) {
    if (!r || !out) return fail(FRT_ERR_INVALID_ARG, "read_scene: null");
    const SceneView& sv = r->sv;
    const void* src = nullptr; size_t bytes = 0;
    switch (which) {
    case 2: src = sv.materials; bytes = (size_t)sv.num_materials * sizeof(MaterialView); break;
    case 3: src = sv.lights; bytes = (size_t)sv.num_lights * sizeof(LightView); break;
    case 4: src = sv.attributes; bytes = (size_t)pool_count(r, kPoolVerts) * sizeof(VertexAttrView); break;
    case 5: src = sv.indices; bytes = (size_t)pool_count(r, kPoolIndices) * sizeof(uint32_t); break;
    case 6: src = sv.mesh_infos; bytes = r->rf.mesh_tris.size() * sizeof(MeshInfoView); break;
    case 18: {      // (made at the first call that needs them: frt_renderer_add_instances, _add_meshes, or this one)
        FRT_DEVICE(r);
        if (const int rc = sync_all(r)) return rc;
        if (const int rc = ensure_normals(r)) return rc;
        src = r->pools.d_normals; bytes = (size_t)pool_count(r, kPoolVerts) * sizeof(float4);
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
