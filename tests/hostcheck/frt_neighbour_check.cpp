// TEST INFRASTRUCTURE ONLY (tests/test_neighbour_fetch.py builds it on demand): the spatial stage's neighbour preparation as the product runs it —
// every word of the neighbour fetched up front, the centre material's is_specular read once per pixel (frt_path.hpp: spatial_neighbor_prepare) —
// against the SEQUENTIAL form of restir_spatial.wgsl:912-982 written out below: position, test, normal + albedo, material, test, reservoir, test.
// Same translation unit as the host-check driver, whose frame buffers hold the inputs the spatial stage of the last rendered frame saw.
#include "frt_hostcheck.cpp"

namespace {

bool valid_sequential(const SceneView& sc, f3 cp, f3 cn, uint32_t cm, f3 pp, f3 pn, uint32_t pm, f3 cam) {   // restir_spatial.wgsl:783-814
    if (cm != pm) return false;
    const MaterialView& mat = sc.materials[cm];
    bool is_specular = mat.roughness < 0.2f || mat.metallic > 0.8f || (mat.transmission > 0.01f);
    if (is_specular) {
        if (dot(cn, pn) < 0.998f) return false;
        if (distance(cp, pp) > 0.01f) return false;
    } else {
        if (dot(cn, pn) < 0.995f) return false;
        float dist_to_camera_sq = dot(cp - cam, cp - cam);
        float threshold = fmaxn(0.00001f, dist_to_camera_sq * 0.001f);
        float dist_diff_sq = dot(cp - pp, cp - pp);
        if (dist_diff_sq > threshold) return false;
    }
    return true;
}

void prepare_sequential(const SceneView& sc, const FrameView& fv, SpatialState& ss, AnyReq& req) {
    ss.pending = false;
    uint32_t px = ss.pix % fv.W, py = ss.pix / fv.W;
    float radius = ss.narrow ? 4.0f : 10.0f;
    float r1 = rand_lcg(ss.local_seed);
    float r2 = rand_lcg(ss.local_seed);
    float angle = 2.0f * kPI * r1;
    float rad = sqrtf_(r2) * radius;
    float sa, ca;
    sincosf_(angle, sa, ca);
    f2 offset = mk2(ca, sa) * rad;
    int nx = (int)px + (int)offset.x, ny = (int)py + (int)offset.y;
    if (nx < 0 || nx >= (int)fv.W || ny < 0 || ny >= (int)fv.H) return;
    uint32_t nidx = (uint32_t)ny * fv.W + (uint32_t)nx;
    float4 n_pos4 = fv.gpos[nidx];
    if (n_pos4.w < 0.0f) return;
    float4 pos_w4 = fv.gpos[ss.pix];
    f3 pos_w = mk3(pos_w4.x, pos_w4.y, pos_w4.z);
    float4 normal_w = fv.gnormal[ss.pix];
    f3 normal = decode_octahedral_normal(normal_w.x, normal_w.y);
    uint32_t mat_id = (uint32_t)(pos_w4.w + 0.1f);
    f3 albedo = xyz(unpack_rgba8(fv.galbedo[ss.pix]));
    f3 camera_pos = mk3(fv.cam.view_pos[0], fv.cam.view_pos[1], fv.cam.view_pos[2]);
    f3 n_pos = mk3(n_pos4.x, n_pos4.y, n_pos4.z);
    float4 n_nrm = fv.gnormal[nidx];
    f3 n_normal = decode_octahedral_normal(n_nrm.x, n_nrm.y);
    uint32_t n_mat_id = (uint32_t)(n_pos4.w + 0.1f);
    f3 n_albedo = xyz(unpack_rgba8(fv.galbedo[nidx]));
    if (!valid_sequential(sc, pos_w, normal, mat_id, n_pos, n_normal, n_mat_id, camera_pos)) return;
    ReservoirView nr = fv.res_temporal[nidx];
    if (nr.p_hat <= 0.0f) return;
    f3 n_s_path = mk3(nr.sx, nr.sy, nr.sz);
    float jacobian = calculate_jacobian(pos_w, normal, albedo, n_s_path, n_pos, n_normal, n_albedo);
    if (ss.narrow) { if (jacobian < 0.5f || jacobian > 2.0f) return; }
    f3 dir_to_v1 = n_s_path - pos_w;
    float dist_to_v1 = length(dir_to_v1);
    if (!(dot(normal, dir_to_v1) > 0.0f)) return;
    if (!(dist_to_v1 > 0.001f)) return;
    f3 ray_dir = normalize(dir_to_v1);
    float dist = fmaxn(dist_to_v1, 0.0f);
    float t_max = fmaxn(dist * 0.999f, 0.0f);
    float t_min = 0.0001f;
    ss.pending = true;
    ss.cand_p_hat = nr.p_hat * jacobian;
    ss.cand_M = nr.M < 20u ? nr.M : 20u;
    ss.cand_weight = ss.cand_p_hat * nr.W * (float)ss.cand_M;
    ss.cand_y = nr.y;
    ss.cand_s_path = n_s_path;
    if (t_min >= t_max) return;
    req.want = true; req.o = pos_w; req.d = ray_dir; req.tmin = t_min; req.tmax = t_max;
}

bool same3(f3 a, f3 b) { return f2u(a.x) == f2u(b.x) && f2u(a.y) == f2u(b.y) && f2u(a.z) == f2u(b.z); }
bool same_reservoir(const ReservoirView& a, const ReservoirView& b) { return memcmp(&a, &b, sizeof(ReservoirView)) == 0; }
// every field of the state that is defined at this point, bit for bit
bool same_state(const SpatialState& a, const SpatialState& b, const AnyReq& ra, const AnyReq& rb) {
    if (!same_reservoir(a.r, b.r) || a.pix != b.pix || a.local_seed != b.local_seed || a.i != b.i || a.n != b.n) return false;
    if (a.narrow != b.narrow || a.pending != b.pending || ra.want != rb.want) return false;
    if (a.pending && (a.cand_y != b.cand_y || a.cand_M != b.cand_M || f2u(a.cand_weight) != f2u(b.cand_weight) ||
                      f2u(a.cand_p_hat) != f2u(b.cand_p_hat) || !same3(a.cand_s_path, b.cand_s_path))) return false;
    if (ra.want && (!same3(ra.o, rb.o) || !same3(ra.d, rb.d) || f2u(ra.tmin) != f2u(rb.tmin) || f2u(ra.tmax) != f2u(rb.tmax))) return false;
    return true;
}

}  // namespace

extern "C" {

// The neighbour loop of every pixel of the frame rendered last (camera `cam`), both forms side by side, each neighbour's visibility ray traced once
// and fed to both. out = {pixels with a surface, neighbour iterations, candidates that reached their ray test, candidates merged, mismatches}.
int nc_compare(void* p, const frt_camera_uniform* cam, unsigned long long out[5]) {
    HostCheck* h = (HostCheck*)p;
    if (h->frame_count == 0) return -1;
    const uint32_t frame = h->frame_count - 1u, cur = frame & 1u;
    const size_t n = (size_t)h->W * h->H;
    std::vector<ReservoirView> res_out(n, zero_reservoir());      // (spatial_begin writes a background pixel's outputs: kept off the renderer's buffers)
    std::vector<uint2> raw_out(n, make_uint2(0, 0));
    FrameView fv{};
    fv.gpos = h->gpos[cur].data(); fv.gnormal = h->gnormal[cur].data(); fv.galbedo = h->galbedo[cur].data();
    fv.res_temporal = h->res[0].data(); fv.res_spatial = res_out.data(); fv.raw = raw_out.data();
    fv.W = h->W; fv.H = h->H; fv.frame_count = frame; fv.max_depth = h->max_depth;
    fv.y0 = 0; fv.y1 = h->H; fv.own_y0 = 0; fv.own_y1 = h->H; fv.prev_y0 = 0; fv.prev_y1 = h->H;
    memcpy(&fv.cam, cam, sizeof(CameraView));
    for (int k = 0; k < 5; ++k) out[k] = 0ull;
    uint32_t stack[kStackDepth];
    for (uint32_t pix = 0; pix < (uint32_t)n; ++pix) {
        PathCtx c(h->sv, fv, stack, 1u);
        SpatialState a, b;
        if (!spatial_begin(c, a, pix)) continue;
        spatial_begin(c, b, pix);
        out[0] += 1;
        const SpatialCentre centre = spatial_centre(h->sv, fv, pix);
        while (a.i < a.n) {
            AnyReq ra, rb;
            ra.want = false; ra.o = splat3(0.0f); ra.d = splat3(0.0f); ra.tmin = 0.0f; ra.tmax = 0.0f;
            rb = ra;
            spatial_neighbor_prepare(c, a, ra, centre);
            prepare_sequential(h->sv, fv, b, rb);
            out[1] += 1;
            if (!same_state(a, b, ra, rb)) { out[4] += 1; break; }
            bool visible = true;
            if (ra.want) { HitRec s; trace<true>(h->sv, ra.o, ra.d, ra.tmin, ra.tmax, stack, 1u, s); visible = s.tri == 0xFFFFFFFFu; }
            if (a.pending) { out[2] += 1; if (visible) out[3] += 1; }
            spatial_neighbor_finish(a, visible);
            spatial_neighbor_finish(b, visible);
        }
        if (!same_reservoir(a.r, b.r)) out[4] += 1;
    }
    return 0;
}

}
