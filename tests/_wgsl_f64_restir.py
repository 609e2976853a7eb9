"""Float64 restatement of the two reservoir passes of the reference, written from the shader text and the Rust bind groups alone:
  * restir.wgsl `main` :842-917 (Phase 2 and 3): reprojection, neighbour validity, albedo correction, M clamp, RIS, final W;
  * restir_spatial.wgsl `main` :857-993: rescale of the centre reservoir, disc sampling, validity, Jacobian, shadow ray, RIS.
Bindings: restir.rs:362-377 binds reservoir_buffers[1] (the previous frame's SPATIAL result) as `prev_reservoirs` and buffers[0] as
`curr_reservoirs`; restir.rs:542-545 picks the G-buffer pair by frame_count % 2 (gbuffer / prev_gbuffer); restir_spatial.rs:349-353 (called from
renderer.rs:292-293) binds buffers[0] as `in_reservoirs` and [1] as `out_reservoirs`; restir_spatial.rs:480-484 writes frame_count to scene_info.y.
Nothing here is shared with the product (csrc/) or the oracle (oracle/). Line numbers are those of the two shaders.

Integer work (pcg_hash, rand_lcg's state and word, the seeds, M) is exact u32 arithmetic. Values that only choose a tap or a branch are formed in
f32 as the shader forms them (prev_uv, prev_uv * size and its vec2u conversion; rand_lcg's float; the disc offset before vec2<i32>()); every value
that flows into an output is float64. The shader's literals are f32 constants: their f32 values are used, so that the only differences left
between this side and an f32 implementation are roundings of operations, which the bounds below count.

`mis` (a set of names) applies one deliberate misreading to this side only (tests/test_wgsl_f64_sensitivity.py):
  "other_reservoirs"   prev_reservoirs is buffers[0]              "temporal_m20"      MAX_RESERVOIR_M_TEMPORAL = 20 (:851)
  "spatial_m16"        min(M, 16) at restir_spatial.wgsl:989       "ratio_inverted"    l_prev / l_curr (:884)
  "ris_le"             rnd * w_sum <= w (:749 / :773)              "normal_0995"       temporal normal threshold 0.995 (:767)
  "no_rescale"         :893-896 dropped                            "jacobian_no_albedo" :845-847 dropped
  "jacobian_clamp_05_2" clamp(jacobian, 0.5, 2.0) (:851)           "offset_rounded"    round() instead of truncation (:921)
  "third_draw_always"  the RIS draw taken for every neighbour      "tmax_dist"         shadow t_max = dist (:389)
  "prev_id_rounded"    prev_id_xy rounded to nearest (:849)
"""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -24                     # unit roundoff of f32
RES = np.dtype([("y", "<u4"), ("w_sum", "<f4"), ("M", "<u4"), ("W", "<f4"), ("s", "<f4", (3,)), ("p_hat", "<f4")])   # restir.wgsl:28-35, 32 bytes
_MASK = np.uint64(0xFFFFFFFF)


def L(x):
    """A shader literal: its f32 value, as float64."""
    return float(f32(x))


LUM = np.array([L(0.2126), L(0.7152), L(0.0722)])

# ---- rounding counts (each division counts 2: an implementation may evaluate a / b as a * (1 / b)). All sums below are sums of non-negative terms,
# so a relative error per operation stays a relative error of the result: the conditioning of luminance + 0.001 and of w_sum is 1. The conditioning
# that is not 1 is that of the two cosines (an absolute error of a unit-vector dot product, divided by the cosine) and is carried per pixel.
N_LUM = 5          # unorm8 / 255 (1), three products (1 each, in parallel), two sums (2), + 0.001 (1)              :882-883, :845-846
N_RATIO = 2 * N_LUM + 2                                     # l_curr / l_prev                                         :884, :847
N_TEMPORAL_P_HAT = N_RATIO + 1                              # prev_r.p_hat * albedo_ratio                             :890
N_TEMPORAL_W_PREV = N_TEMPORAL_P_HAT + 2                    # * prev_r.W * f32(clamped_M) (f32(M) is exact)           :894
N_TEMPORAL_W_SUM = N_TEMPORAL_W_PREV + 1                    # p_hat + w_prev                                          :747
N_TEMPORAL_W = N_TEMPORAL_P_HAT + N_TEMPORAL_W_SUM + 5      # (1 / p_hat_final) * (w_sum / f32(M))                    :910
N_COS = 14         # octahedral decode + normalize (6), normalize(dir) (5), dot (3): ABSOLUTE error N_COS * EPS of a cosine  :833, :836
N_JACOBIAN = N_RATIO + 2 + 1                                # cos_curr / cos_neigh (2), * ratio (1); + N_COS * EPS * (1 / cos_curr + 1 / cos_neigh)
N_SPATIAL_WEIGHT = 3                                        # neighbor_r.p_hat * jacobian * W * f32(M_new)            :988-990
N_RESCALE = 3                                               # w_sum * (20 / f32(M))                                   :894
BAND = 16 * EPS    # a comparison is undecided when its two sides are closer than this (relative; absolute for cosines of unit vectors)


def pcg_hash(x):                                             # restir.wgsl:132-136
    x = np.asarray(x, np.uint64) & _MASK
    state = (x * np.uint64(747796405) + np.uint64(2891336453)) & _MASK
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & _MASK
    return ((word >> np.uint64(22)) ^ word) & _MASK


def rand_lcg(state):                                         # restir.wgsl:781-786: -> (new state, f32 value)
    state = (np.asarray(state, np.uint64) * np.uint64(747796405) + np.uint64(2891336453)) & _MASK
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & _MASK
    out = ((word >> np.uint64(22)) ^ word) & _MASK
    return state, out.astype(np.uint32).astype(f32) / f32(4294967295.0)


def _normalize(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def decode_octahedral(e):                                    # restir.wgsl:152-158
    e = np.asarray(e, np.float64)
    n = np.stack([e[..., 0], e[..., 1], 1.0 - np.abs(e[..., 0]) - np.abs(e[..., 1])], -1)
    t = np.maximum(-n[..., 2], 0.0)
    n[..., 0] += np.where(n[..., 0] >= 0.0, -t, t)
    n[..., 1] += np.where(n[..., 1] >= 0.0, -t, t)
    return _normalize(n)


def luminance(c):                                            # restir.wgsl:742-744
    return c @ LUM


def _mat_id(w):                                              # u32(pos.w + 0.1), in f32 (:861, :865)
    return (np.asarray(w, f32) + f32(0.1)).astype(np.int64)


def _specular(materials, mat_id, r_lim, m_lim, t_lim):
    """roughness < r_lim || metallic > m_lim || transmission > t_lim: f32 fields against f32 literals, exact (Material, restir.wgsl:37-49)."""
    m = materials.view(f32)[np.clip(mat_id, 0, len(materials) - 1)]
    return (m[..., 7] < f32(r_lim)) | (m[..., 8] > f32(m_lim)) | (m[..., 9] > f32(t_lim))


def _near(a, b, rel=BAND):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))


# ------------------------------------------------------------------------------------------------ restir.wgsl main, :842-917
def temporal_merge_f64(inp, W, H, frame_count, view_pos, materials, mis=()):
    """inp, as read back: gpos / gnormal (H, W, 4) f32 and galbedo (H, W, 4) u8 of the current slot, gpos_prev / gnormal_prev / galbedo_prev of the
    other one, motion (H, W, 2) f32, prev_res (H, W) RES (buffers[1]), temporal_res (H, W) RES (buffers[0] before the pass: read only under
    "other_reservoirs"), cand (H, W, 4) f32 = (v1_pos, p_hat) of the fresh candidate. Returns a dict of (H, W) arrays: y, M (exact), w_sum, W, p_hat
    (float64) and their bounds *_tol, sel (0 the zero path, 1 the candidate's v1, 2 the history's s_path), ambiguous (a validity / window decision
    within f32 rounding of its threshold), ris_amb (the RIS draw alone is) and, for those, the other outcome under alt_*."""
    n = W * H
    idx = np.arange(n, dtype=np.uint64)
    xs, ys = (idx % np.uint64(W)).astype(np.int64), (idx // np.uint64(W)).astype(np.int64)
    gpos = inp["gpos"].reshape(n, 4); pos = gpos[:, :3].astype(np.float64)
    bg = gpos[:, 3] < 0                                                                               # :805
    cand = inp["cand"].reshape(n, 4).astype(np.float64)
    seed_base = (idx + np.uint64(frame_count) * np.uint64(927163)) & _MASK                            # :797
    y_cand = pcg_hash(seed_base)                                                                      # :798
    # Phase 1 (:833-840): update_reservoir(r, seed_candidate, p_hat, 0.5, 1, p_hat, v1_pos) on the zero reservoir
    p_c = cand[:, 3]
    took_c = 0.5 * p_c < p_c
    w_sum = p_c.copy(); M = np.ones(n, np.int64)
    y = np.where(took_c, y_cand, 0); p_hat = np.where(took_c, p_c, 0.0); sel = np.where(took_c, 1, 0)
    # Phase 2 (:846-900)
    size = np.array([W, H], f32)
    uv = (np.stack([xs, ys], -1).astype(f32) + f32(0.5)) / size                                       # :847
    with np.errstate(invalid="ignore", over="ignore"):
        prev_uv = uv + inp["motion"].reshape(n, 2).astype(f32)                                        # :848
        inside = (prev_uv[:, 0] >= 0) & (prev_uv[:, 0] <= 1) & (prev_uv[:, 1] >= 0) & (prev_uv[:, 1] <= 1)   # :854
        pf = np.where(inside[:, None], prev_uv * size, f32(0))
    q = (np.floor(pf + f32(0.5)) if "prev_id_rounded" in mis else np.floor(pf)).astype(np.int64)     # :849 vec2u(): truncation (pf >= 0)
    tex_ok = inside & (q[:, 0] < W) & (q[:, 1] < H)                  # textureLoad beyond the size returns zeros (prev_uv == 1)
    qi = np.where(tex_ok, q[:, 1] * W + q[:, 0], 0)
    lin = q[:, 1] * W + q[:, 0]                                      # :855; the storage buffer is indexed linearly: in range it reads that element
    res_ok = inside & (lin < n)
    z = lambda a: np.where(tex_ok.reshape((n,) + (1,) * (a.ndim - 1)), a, 0)
    ppos4 = z(inp["gpos_prev"].reshape(n, 4)[qi]); pnrm = z(inp["gnormal_prev"].reshape(n, 4)[qi]); palb = z(inp["galbedo_prev"].reshape(n, 4)[qi])
    cur_mat, prev_mat = _mat_id(gpos[:, 3]), _mat_id(ppos4[:, 3])                                     # :861, :865
    cn, pn = decode_octahedral(inp["gnormal"].reshape(n, 4)[:, :2]), decode_octahedral(pnrm[:, :2])
    spec = _specular(materials, cur_mat, 0.2, 0.8, 0.01)                                              # :870
    # is_valid_neighbor (:758-778)
    ndot = (cn * pn).sum(-1)
    nthr = L(0.995) if "normal_0995" in mis else L(0.99)
    ppos = ppos4[:, :3].astype(np.float64)
    dds = ((pos - ppos) ** 2).sum(-1)
    thr = np.maximum(L(0.00001), ((pos - np.asarray(view_pos, np.float64)[:3]) ** 2).sum(-1) * L(0.001))
    same = cur_mat == prev_mat
    valid = inside & ~bg & same & ~(ndot < nthr) & ~(dds > thr) & ~spec
    reach = inside & ~bg & same & ~spec                              # the float tests are only taken (and only matter) here
    amb = reach & (np.abs(ndot - nthr) <= BAND)
    amb |= reach & ~(ndot < nthr) & _near(dds, thr)
    # :877-898
    src = inp["temporal_res"] if "other_reservoirs" in mis else inp["prev_res"]
    pr = src.reshape(n)[np.where(res_ok, lin, 0)]
    pr_p = np.where(res_ok, pr["p_hat"].astype(np.float64), 0.0); pr_W = np.where(res_ok, pr["W"].astype(np.float64), 0.0)
    pr_M = np.where(res_ok, pr["M"].astype(np.int64), 0); pr_y = np.where(res_ok, pr["y"].astype(np.uint64), 0)
    l_curr = luminance(inp["galbedo"].reshape(n, 4)[:, :3] / 255.0) + L(0.001)                        # :882
    l_prev = luminance(palb[:, :3] / 255.0) + L(0.001)                                                # :883
    ratio = l_prev / l_curr if "ratio_inverted" in mis else l_curr / l_prev                           # :884
    window = (ratio < L(3.0)) & (ratio > L(0.33))                                                     # :888
    amb |= valid & (_near(ratio, L(3.0)) | _near(ratio, L(0.33)))
    p_new = pr_p * ratio                                                                              # :890
    amb |= valid & window & (p_new > 0) & (p_new < 2e-38)            # an f32 product this small may round to zero
    merge = valid & window & (p_new > 0)                                                              # :892
    cM = np.minimum(pr_M, 20 if "temporal_m20" in mis else 16)                                        # :893
    w_prev = np.where(merge, p_new * pr_W * cM, 0.0)                                                  # :894
    _, rnd = rand_lcg(seed_base)                                                                      # :896 (local_seed = seed_base, :801)
    rnd = rnd.astype(np.float64)
    w_sum2 = w_sum + w_prev                                                                           # :747
    lhs = rnd * w_sum2
    with np.errstate(invalid="ignore"):
        took_h = merge & ((lhs <= w_prev) if "ris_le" in mis else (lhs < w_prev))                     # :749
        ris_amb = merge & (np.abs(lhs - w_prev) <= (N_TEMPORAL_W_SUM + 2) * EPS * np.maximum(np.abs(lhs), np.abs(w_prev))) & ~(w_prev == 0)
    ris_amb &= ~amb

    def finish(took):
        o = {"w_sum": np.where(merge, w_sum2, w_sum), "M": np.where(merge, M + cM, M)}
        o["y"] = np.where(took, pr_y, y); o["sel"] = np.where(took, 2, sel)
        ph = np.where(took, p_new, p_hat)
        with np.errstate(divide="ignore", invalid="ignore"):
            o["W"] = np.where(ph > 0, (1.0 / ph) * (o["w_sum"] / o["M"]), 0.0)                        # :907-915
        o["p_hat"] = np.where(ph > 0, ph, 0.0)
        for k in o:
            o[k] = np.where(bg, 0, o[k])                                                              # :805-811
        return o
    out = finish(took_h)
    alt = finish(took_h ^ ris_amb)
    for k in ("y", "sel", "W", "p_hat"):
        out["alt_" + k] = alt[k]
    hist = out["sel"] == 2
    out["w_sum_tol"] = np.where(merge, N_TEMPORAL_W_SUM, 0) * EPS * np.abs(out["w_sum"])
    out["p_hat_tol"] = np.where(hist, N_TEMPORAL_P_HAT, 0) * EPS * np.abs(out["p_hat"])
    out["W_tol"] = np.where(merge, N_TEMPORAL_W, 5) * EPS * np.abs(out["W"])
    out["alt_p_hat_tol"] = N_TEMPORAL_P_HAT * EPS * np.abs(out["alt_p_hat"]); out["alt_W_tol"] = N_TEMPORAL_W * EPS * np.abs(out["alt_W"])
    out["ambiguous"] = amb; out["ris_amb"] = ris_amb; out["merged"] = merge; out["prev_index"] = np.where(res_ok, lin, -1)
    return {k: v.reshape(H, W) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ trace_shadow_ray, restir_spatial.wgsl:380-400
def _any_hit(tris, origins, dirs, tmin, tmax, eps=1e-5, budget=3_000_000):
    """Any-hit variant of _wgsl_f64._closest_hit (RayDesc flags 0x4: the first opaque hit ends the query; both faces; every triangle is opaque),
    brute force in float64, one origin per ray. Returns (occluded, ambiguous): ambiguous when some triangle is met within `eps` of one of its edges
    (barycentric) or within the t band of an end of (tmin, tmax), i.e. where an f32 tracer may decide the other way."""
    T = tris.astype(np.float64)
    v0, e1, e2 = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    n = len(dirs)
    occ = np.zeros(n, bool); amb = np.zeros(n, bool)
    chunk = max(1, budget // max(len(T), 1))
    for s in range(0, n, chunk):
        d = dirs[s:s + chunk, None, :]; o = origins[s:s + chunk, None, :]
        lo, hi = tmin[s:s + chunk, None], tmax[s:s + chunk, None]
        p = np.cross(d, e2[None])
        det = (p * e1[None]).sum(-1)
        tvec = o - v0[None]
        qv = np.cross(tvec, e1[None])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u = (tvec * p).sum(-1) * inv
            v = (d * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
            occ[s:s + chunk] = ((det != 0.0) & (t > lo) & (t < hi) & (margin >= 0.0)).any(1)
            band_lo, band_hi = eps * (1.0 + lo), eps * hi
            in_t = (t > lo - band_lo) & (t < hi + band_hi)
            edge = in_t & (np.abs(margin) < eps)
            ends = (margin > -eps) & ((np.abs(t - lo) < band_lo) | (np.abs(t - hi) < band_hi))
            amb[s:s + chunk] = ((det != 0.0) & (edge | ends)).any(1)
    return occ, amb


_SHADOW = {}


# ------------------------------------------------------------------------------------------------ restir_spatial.wgsl main, :857-993
def spatial_reuse_f64(inp, W, H, frame_word, view_pos, materials, tris, mis=()):
    """inp, as read back: gpos / gnormal (H, W, 4) f32, galbedo (H, W, 4) u8, in_res (H, W) RES (buffers[0]). frame_word: scene_info.y. tris: the
    scene's world-space triangles (v0, e1, e2). Returns (H, W) arrays: y, M (exact), w_sum with w_sum_tol — the reservoir after the neighbour loop
    (:993), of which only these three reach out_reservoirs — background, merges (neighbours merged) and ambiguous."""
    n = W * H
    idx = np.arange(n, dtype=np.int64)
    xs, ys = idx % W, idx // W
    gpos = inp["gpos"].reshape(n, 4); pos = gpos[:, :3].astype(np.float64)
    bg = gpos[:, 3] < 0                                                                               # :874
    nrm = decode_octahedral(inp["gnormal"].reshape(n, 4)[:, :2])                                      # :887
    mat = _mat_id(np.where(bg, f32(0), gpos[:, 3]))                                                   # :888
    alb = inp["galbedo"].reshape(n, 4)[:, :3] / 255.0                                                 # :889
    lum = luminance(alb) + L(0.001)
    res = inp["in_res"].reshape(n)
    r_y = res["y"].astype(np.uint64); r_w = res["w_sum"].astype(np.float64); r_M = res["M"].astype(np.int64)
    r_tol = np.zeros(n)
    big = r_M > 20                                                                                    # :893-896
    if "no_rescale" not in mis:
        with np.errstate(invalid="ignore"):
            r_w = np.where(big, r_w * (20.0 / np.maximum(r_M, 1)), r_w)
        r_tol = np.where(big, N_RESCALE * EPS * np.abs(r_w), 0.0)
        r_M = np.where(big, 20, r_M)
    seed = (idx.astype(np.uint64) + np.uint64(frame_word) * np.uint64(0x12345678)) & _MASK           # :866, :870
    narrow = _specular(materials, mat, 0.1, 0.9, 0.1)                                                 # :906, :957
    v_spec = _specular(materials, mat, 0.2, 0.8, 0.01)                                                # :792 (the centre's material: the ids are equal there)
    count = np.where(narrow, 3, 5)
    radius = np.where(narrow, f32(4.0), f32(10.0)).astype(f32)
    cam = np.asarray(view_pos, np.float64)[:3]
    thr = np.maximum(L(0.00001), ((pos - cam) ** 2).sum(-1) * L(0.001))                               # :806-808
    amb = np.zeros(n, bool); merges = np.zeros(n, np.int64)
    two_pi = f32(2.0) * f32(3.14159265359)
    for i in range(5):                                                                                # :912
        live = ~bg & (i < count)
        seed1, r1 = rand_lcg(seed); seed2, r2 = rand_lcg(seed1)                                       # :914-915
        seed = np.where(live, seed2, seed)
        if "third_draw_always" in mis:
            seed3, rnd_all = rand_lcg(seed)
            seed = np.where(live, seed3, seed)
        angle = two_pi * r1                                                                           # :918, f32
        rad = np.sqrt(r2) * radius                                                                    # :919, f32 (sqrt is correctly rounded)
        off = np.stack([np.cos(angle.astype(np.float64)).astype(f32), np.sin(angle.astype(np.float64)).astype(f32)], -1) * rad[:, None]   # :920
        off64 = off.astype(np.float64)
        step = np.rint(off64) if "offset_rounded" in mis else np.trunc(off64)                         # :921 vec2<i32>(): toward zero
        nearest = np.rint(off64)
        amb |= live & ((np.abs(off64 - nearest) < 1e-4) & (nearest != 0)).any(-1)                     # (0 is no boundary of a truncation)
        nx, ny = xs + step[:, 0].astype(np.int64), ys + step[:, 1].astype(np.int64)
        go = live & (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)                                       # :924
        ni = np.where(go, ny * W + nx, 0)
        npos4 = gpos[ni]
        go &= ~(npos4[:, 3] < 0)                                                                      # :932
        npos = npos4[:, :3].astype(np.float64)
        nn = nrm[ni]; nmat = _mat_id(np.where(go, npos4[:, 3], f32(0)))
        go &= nmat == mat                                                                             # :789
        ndot = (nrm * nn).sum(-1)
        nthr = np.where(v_spec, L(0.998), L(0.995))                                                   # :796, :803
        amb |= go & (np.abs(ndot - nthr) <= BAND)
        go &= ~(ndot < nthr)
        dds = ((pos - npos) ** 2).sum(-1)
        dist = np.sqrt(dds)
        amb |= go & np.where(v_spec, _near(dist, L(0.01)), _near(dds, thr))
        go &= np.where(v_spec, ~(dist > L(0.01)), ~(dds > thr))                                       # :800, :810
        nr = res[ni]
        go &= ~(nr["p_hat"] <= 0)                                                                     # :942, f32, exact
        sp = nr["s"].astype(np.float64)
        # calculate_jacobian (:822-854)
        dir_c, dir_n = sp - pos, sp - npos
        with np.errstate(invalid="ignore", divide="ignore"):
            cos_c = np.maximum((nrm * _normalize(dir_c)).sum(-1), 0.0)
            cos_n = np.maximum((nn * _normalize(dir_n)).sum(-1), 0.0)
            cos_c = np.where(np.isfinite(cos_c), cos_c, 0.0); cos_n = np.where(np.isfinite(cos_n), cos_n, 0.0)   # normalize(0): undefined, crafted as such nowhere the result is used
            low = cos_n <= L(0.001)                                                                   # :838
            amb |= go & (np.abs(cos_n - L(0.001)) <= N_COS * EPS)
            jac = cos_c / cos_n
            if "jacobian_no_albedo" not in mis:
                jac = jac * (lum / (luminance(inp["galbedo"].reshape(n, 4)[ni][:, :3] / 255.0) + L(0.001)))   # :845-847
            jrel = (N_JACOBIAN * EPS + N_COS * EPS * (1.0 / cos_c + 1.0 / cos_n))
            jrel = np.where(np.isfinite(jrel), jrel, np.inf)
        c_lo, c_hi = (L(0.5), L(2.0)) if "jacobian_clamp_05_2" in mis else (L(0.1), L(10.0))
        with np.errstate(invalid="ignore"):
            clamped = (jac < c_lo * (1 - np.minimum(jrel, 1.0))) | (jac > c_hi * (1 + jrel))          # safely outside: the clamp's constant, no error
            jc = np.where(low, 0.0, np.clip(np.where(np.isnan(jac), c_lo, jac), c_lo, c_hi))          # :851 (cos_curr = 0 with a live cos_neigh: 0 -> 0.1)
            jrel = np.where(low | clamped, 0.0, jrel)
            # the specular centre's window (:957-964); jac is then within [0.1, 10] unless it is 0
            lim_amb = narrow & ~low & ((np.abs(jc - L(0.5)) <= jrel * L(0.5)) | (np.abs(jc - L(2.0)) <= jrel * L(2.0)))
        amb |= go & lim_amb
        go &= ~(narrow & ((jc < L(0.5)) | (jc > L(2.0))))
        # visibility (:965-984)
        dlen = np.sqrt((dir_c ** 2).sum(-1))
        nd = (nrm * dir_c).sum(-1)
        amb |= go & (np.abs(nd) <= BAND * dlen)
        amb |= go & (nd > 0) & _near(dlen, L(0.001))
        ray = go & (nd > 0) & (dlen > L(0.001))                                                       # :969, :971
        k = np.nonzero(ray)[0]
        vis = np.zeros(n, bool)
        if len(k):
            tmax = np.maximum(dlen[k] * (1.0 if "tmax_dist" in mis else L(0.999)), 0.0)               # :389
            tmin = np.full(len(k), L(0.0001))                                                         # :385 (t_min >= t_max cannot happen: dist > 0.001)
            o, d = pos[k], dir_c[k] / dlen[k][:, None]
            key = (id(tris), o.tobytes(), d.tobytes(), tmax.tobytes())
            if key not in _SHADOW:
                if len(_SHADOW) > 64:
                    _SHADOW.clear()
                _SHADOW[key] = _any_hit(tris, o, d, tmin, tmax)
            occ, ramb = _SHADOW[key]
            vis[k] = ~occ
            amb[k] |= ramb
        go &= vis                                                                                     # :984
        # :988-992
        p_corr = nr["p_hat"].astype(np.float64) * jc
        M_new = np.minimum(nr["M"].astype(np.int64), 16 if "spatial_m16" in mis else 20)
        weight = p_corr * nr["W"].astype(np.float64) * M_new
        if "third_draw_always" in mis:
            rnd = rnd_all
        else:
            seed3, rnd = rand_lcg(seed)
            seed = np.where(go, seed3, seed)
        rnd = rnd.astype(np.float64)
        w_rel = jrel + N_SPATIAL_WEIGHT * EPS
        with np.errstate(invalid="ignore"):
            new_w = r_w + weight
            new_tol = r_tol + np.abs(weight) * np.where(np.isfinite(w_rel), w_rel, 1.0) + EPS * np.abs(new_w)
            lhs = rnd * new_w
            take = (lhs <= weight) if "ris_le" in mis else (lhs < weight)                             # :773
            amb |= go & (np.abs(lhs - weight) <= new_tol + 2 * EPS * np.abs(weight)) & ~(weight == 0)     # (0 < 0 is false under any rounding)
        r_w = np.where(go, new_w, r_w); r_tol = np.where(go, new_tol, r_tol)
        r_M = np.where(go, r_M + M_new, r_M)
        r_y = np.where(go & take, nr["y"].astype(np.uint64), r_y)
        merges += go
    out = {"y": np.where(bg, 0, r_y), "M": np.where(bg, 0, r_M), "w_sum": np.where(bg, 0.0, r_w), "w_sum_tol": np.where(bg, 0.0, r_tol),
           "background": bg, "ambiguous": amb & ~bg, "merges": merges, "narrow": narrow & ~bg}
    return {k: v.reshape(H, W) for k, v in out.items()}
