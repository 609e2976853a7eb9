"""Float64 restatement of the two deterministic passes of the reference, written from the shader text alone:
  * gbuffer.wgsl `main` (:91-255): camera ray, closest hit, normal / tangent frame, textures, motion vector;
  * post.wgsl `main` (:61-282): bilateral filter, variance clipping in YCoCg, history reprojection, blend, tonemap, gamma.
Line numbers below are those of the two shaders. Nothing here is shared with the product (csrc/) or the oracle (oracle/): it is the
independent side of tests/test_wgsl_f64_*.py, which compare both implementations against it pixel by pixel.

`mis` (a set of names) applies one deliberate misreading of the shader to this side only; tests/test_wgsl_f64_sensitivity.py uses it to
prove that the comparisons are tight enough to notice each of them:
  "m_inv_transposed"  normal_w = m_inv * n instead of n * m_inv (:159)      "tbn_transposed"    TBN_ff^T * n instead of TBN_ff * n (:218)
  "motion_sign"       curr_uv - prev_uv instead of prev_uv - curr_uv (:242)  "no_y_flip"         ndc * (0.5, 0.5) + 0.5 for the motion uv (:239-240)
  "oct_sign"          sign() instead of select(-1, 1, x >= 0) (:54-55)      "clamp_to_edge"     clamp-to-edge instead of Repeat addressing
  "history_clamped"   off-image history taps read the nearest pixel instead of 0 (post.wgsl:219-222)
  "speed_le"          speed <= 0.5 instead of speed < 0.5 (post.wgsl:247)
"""
import numpy as np

TEX = 1024
CAM_BYTES = 288


# ------------------------------------------------------------------------------------------------ camera (gbuffer.wgsl:4-12)
def camera_f64(cam):
    """CameraUniform bytes -> dict of float64 row-major 4x4 matrices (the uniform stores mat4x4f column by column)."""
    b = np.frombuffer(bytes(cam), np.uint8)[:CAM_BYTES]
    f = b[:272].view(np.float32).astype(np.float64)
    m = lambda k: f[16 * k:16 * k + 16].reshape(4, 4).T
    u = b[272:280].view(np.uint32)
    return {"view_proj": m(0), "view_inverse": m(1), "proj_inverse": m(2), "view_pos": f[48:52], "prev_view_proj": f[52:68].reshape(4, 4).T,
            "frame_count": int(u[0]), "num_lights": int(u[1])}


def scene_arrays(scene):
    """The scene tables both libraries expose under the same names (frt.SceneBuilder.get / OrcScene.get)."""
    return {k: scene.get(k) for k in ("tris", "tri_instance", "instances", "attributes", "indices", "mesh_infos", "materials")}


def default_textures():
    """builder.rs add_default_textures: colour layers white, 64-texel checker, black; data layers white, flat normal (128, 128, 255), black."""
    white = np.full((TEX, TEX, 4), 255, np.uint8)
    black = np.zeros((TEX, TEX, 4), np.uint8); black[..., 3] = 255
    y, x = np.mgrid[0:TEX, 0:TEX]
    checker = np.where((((x // 64) + (y // 64)) % 2 == 0)[..., None], white, black)
    flat = np.empty((TEX, TEX, 4), np.uint8); flat[...] = (128, 128, 255, 255)
    return {"color": [white, checker, black], "data": [white, flat, black]}


# ------------------------------------------------------------------------------------------------ helpers
def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def decode_octahedral(e):                           # gbuffer.wgsl:38-44, post.wgsl:28-34
    e = np.asarray(e, np.float64)
    n = np.stack([e[..., 0], e[..., 1], 1.0 - np.abs(e[..., 0]) - np.abs(e[..., 1])], -1)
    t = np.maximum(-n[..., 2], 0.0)
    n[..., 0] += np.where(n[..., 0] >= 0.0, -t, t)
    n[..., 1] += np.where(n[..., 1] >= 0.0, -t, t)
    return _normalize(n)


def encode_octahedral(n, mis=()):                   # gbuffer.wgsl:46-62
    l1 = np.abs(n).sum(-1)
    res = np.where((l1 > 0.0)[..., None], n[..., :2] * (1.0 / np.maximum(l1, 1e-6))[..., None], 0.0)
    x, y = res[..., 0], res[..., 1]
    if "oct_sign" in mis:
        sx, sy = np.sign(x), np.sign(y)
    else:
        sx, sy = np.where(x >= 0.0, 1.0, -1.0), np.where(y >= 0.0, 1.0, -1.0)
    fold = np.stack([(1.0 - np.abs(y)) * sx, (1.0 - np.abs(x)) * sy], -1)
    return np.where((n[..., 2] < 0.0)[..., None], fold, res)


def srgb_to_linear(c8):
    """The sRGB transfer function, exact (Rgba8UnormSrgb texel decode)."""
    c = np.asarray(c8, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def sample_level0(layer, srgb, uv, mis=()):
    """textureSampleLevel(..., uv, layer, 0.0) under the sampler of renderer.rs:240-249: Linear filtering between texel centres, Repeat
    addressing; the colour array decodes sRGB per texel before filtering. layer: (1024, 1024, 4) uint8. uv: (..., 2) float64."""
    tex = np.concatenate([srgb_to_linear(layer[..., :3]), layer[..., 3:] / 255.0], -1) if srgb else layer / 255.0
    x = uv[..., 0] * TEX - 0.5
    y = uv[..., 1] * TEX - 0.5
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[..., None], (y - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    if "clamp_to_edge" in mis:
        wrap = lambda i: np.clip(i, 0, TEX - 1)
    else:
        wrap = lambda i: np.mod(i, TEX)
    t = lambda xi, yi: tex[wrap(yi), wrap(xi)]
    top = t(x0, y0) * (1 - ax) + t(x0 + 1, y0) * ax
    bot = t(x0, y0 + 1) * (1 - ax) + t(x0 + 1, y0 + 1) * ax
    return top * (1 - ay) + bot * ay


# ------------------------------------------------------------------------------------------------ closest hit
def _closest_hit(sc, origin, dirs, tmin=0.001, tmax=1000.0, eps=1e-5, chunk=4096):
    """Brute force over every world-space triangle (rayQueryProceed with flags 0: nearest opaque hit, both faces), float64.
    Returns tri (-1 = miss), t, barycentrics (u, v), determinant sign, and the ambiguity mask: some triangle whose hit float64 cannot
    decide robustly — within `eps` of one of its edges (barycentric) at a t that could be the nearest, or a second hit within eps * t —
    and the part of it where the ray passes within f32 rounding (1e-6) of an edge (no precision decides those: the tracer's tie rule does)."""
    T = sc["tris"].astype(np.float64)
    v0, e1, e2 = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    n = dirs.shape[0]
    tri = np.full(n, -1, np.int64); tt = np.full(n, np.inf); uu = np.zeros(n); vv = np.zeros(n); det_out = np.zeros(n)
    amb = np.zeros(n, bool); exact = np.zeros(n, bool)
    o = origin[None, None, :]
    tvec = o - v0[None]                                   # [1, T, 3]
    qv = np.cross(tvec, e1[None])                         # [1, T, 3]
    for s in range(0, n, chunk):
        d = dirs[s:s + chunk, None, :]                    # [P, 1, 3]
        p = np.cross(d, e2[None])
        det = (p * e1[None]).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u = (tvec * p).sum(-1) * inv
            v = (d * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        ok_t = (t > tmin) & (t < tmax) & (det != 0.0)
        hit = ok_t & (margin >= 0.0)
        th = np.where(hit, t, np.inf)
        k = np.argmin(th, axis=1)
        r = np.arange(len(k))
        best = th[r, k]
        got = np.isfinite(best)
        tri[s:s + chunk] = np.where(got, k, -1)
        tt[s:s + chunk] = best
        uu[s:s + chunk] = u[r, k]; vv[s:s + chunk] = v[r, k]; det_out[s:s + chunk] = det[r, k]
        lim = np.where(got, best * (1.0 + eps), np.inf)[:, None]
        near_edge = ok_t & (np.abs(margin) < eps) & (t <= lim)
        th2 = th.copy(); th2[r, k] = np.inf
        second = th2.min(axis=1)
        with np.errstate(invalid="ignore"):
            amb[s:s + chunk] = near_edge.any(axis=1) | (got & (second - best < eps * best))
        exact[s:s + chunk] = (near_edge & (np.abs(margin) < 1e-6)).any(axis=1)
    return tri, tt, uu, vv, det_out, amb, exact


# ------------------------------------------------------------------------------------------------ gbuffer.wgsl main
_HITS = {}


def gbuffer_f64(sc, cam, W, H, textures, mis=(), uv_delta=2e-5):
    """sc: scene_arrays(); cam: CameraUniform bytes; textures: {"color": [layers], "data": [layers]} as the scene holds them.
    Returns a dict of float64 arrays shaped (H, W, ...): pos, mat_id (-1 = miss), normal (final_normal), enc_normal, uv, albedo
    (before unorm8), motion, miss, ambiguous, on_edge (the ambiguous pixels whose ray meets an edge to within 1e-6); t and cos (|cosine| between the ray and the triangle's plane normal) of the hit; and
    albedo_sens / normal_sens, the largest change of albedo / encoded normal when uv moves by uv_delta along u or v."""
    c = camera_f64(cam)
    ys, xs = np.mgrid[0:H, 0:W]
    uv = (np.stack([xs, ys], -1).reshape(-1, 2) + 0.5) / np.array([W, H], np.float64)            # :97
    ndc = np.stack([uv[:, 0] * 2.0 - 1.0, 1.0 - uv[:, 1] * 2.0], -1)                               # :98
    vi, pi = c["view_inverse"], c["proj_inverse"]
    origin = vi[:3, 3]                                                                              # :103 view_inv[3].xyz
    h = np.concatenate([ndc, np.ones((len(ndc), 2))], -1)
    tgt = h @ (vi @ pi).T                                                                           # :104
    dirs = _normalize(tgt[:, :3] / tgt[:, 3:4] - origin)                                           # :105
    key = (hash(sc["tris"].tobytes()), dirs.tobytes(), origin.tobytes())    # the hits do not depend on `mis`: computed once per ray set
    if key not in _HITS:
        _HITS.clear()
        _HITS[key] = _closest_hit(sc, origin, dirs)
    tri, t, bu, bv, det, amb, exact = _HITS[key]
    n = len(tri)
    out = {"pos": np.zeros((n, 3)), "mat_id": np.full(n, -1.0), "normal": np.zeros((n, 3)), "enc_normal": np.zeros((n, 2)),
           "uv": np.zeros((n, 2)), "albedo": np.zeros((n, 3)), "motion": np.zeros((n, 2)), "miss": tri < 0, "ambiguous": amb, "on_edge": exact,
           "t": np.where(tri >= 0, t, 0.0), "cos": np.ones(n), "albedo_sens": np.zeros((n, 3)), "normal_sens": np.zeros((n, 2))}
    hitm = tri >= 0
    k = np.nonzero(hitm)[0]
    if len(k):
        g = tri[k]
        inst = sc["instances"][sc["tri_instance"][g]]
        mesh_id, mat_id, first = inst[:, 0].astype(np.int64), inst[:, 1].astype(np.int64), inst[:, 2].astype(np.int64)
        M = inst[:, 5:21].view(np.float32).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)   # column-major -> row-major
        A = M[:, :3, :3]
        m_inv = np.linalg.inv(A)                     # world_to_object's 3x3 (:155-156)
        prim = g - first                             # committed.primitive_index
        mi = sc["mesh_infos"][mesh_id].astype(np.int64)
        base = mi[:, 1] + prim * 3                   # :130
        att = sc["attributes"].astype(np.float64)
        ix = [sc["indices"][base + j].astype(np.int64) + mi[:, 0] for j in range(3)]                 # :131-133
        v = [att[i] for i in ix]
        u_b, v_b = bu[k], bv[k]                      # committed.barycentrics (:147-149)
        w_b = 1.0 - u_b - v_b
        bary = lambda a0, a1, a2: a0 * w_b[:, None] + a1 * u_b[:, None] + a2 * v_b[:, None]
        nrm = [decode_octahedral(vk[:, 0:2]) for vk in v]                                           # :139-141
        local_normal = _normalize(bary(*nrm))                                                       # :151
        local_tangent = _normalize(bary(*[vk[:, 4:7] for vk in v]))                                 # :152
        if "m_inv_transposed" in mis:
            row = lambda x: np.einsum("pij,pj->pi", m_inv, x)
        else:
            row = lambda x: np.einsum("pj,pji->pi", x, m_inv)    # row vector times matrix: out[i] = dot(x, column i)
        normal_w = _normalize(row(local_normal))                                                    # :159
        tangent_w = _normalize(row(local_tangent))                                                  # :160
        # front face: counter-clockwise seen from the ray in object space; the world triangle's winding flips under a mirroring instance
        front = (det[k] > 0.0) ^ (np.linalg.det(A) < 0.0)
        ffnormal = np.where(front[:, None], normal_w, -normal_w)                                    # :169
        pos = origin + dirs[k] * t[k][:, None]                                                      # :171
        mat = sc["materials"][mat_id]
        matf = mat.view(np.float32).astype(np.float64)
        tex_uv = bary(*[vk[:, 2:4] for vk in v])                                                    # :174
        tid0, nid0, oid = mat[:, 12] & 0xFFFF, mat[:, 12] >> 16, mat[:, 13] & 0xFFFF

        def textured(tuv):
            """albedo and final_normal at texture coordinate tuv (:178-221)."""
            tex_color = np.ones((len(k), 4))
            occlusion = np.ones(len(k))
            normal_local = np.tile([0.0, 0.0, 1.0], (len(k), 1))
            for layer in np.unique(tid0[tid0 != 0xFFFF]):                                           # :182-184
                s = tid0 == layer
                tex_color[s] = sample_level0(textures["color"][layer], True, tuv[s], mis)
            for layer in np.unique(oid[oid != 0xFFFF]):                                             # :191-193
                s = oid == layer
                occlusion[s] = sample_level0(textures["data"][layer], False, tuv[s], mis)[:, 0]
            for layer in np.unique(nid0[nid0 != 0xFFFF]):                                           # :199-202
                s = nid0 == layer
                normal_local[s] = _normalize(sample_level0(textures["data"][layer], False, tuv[s], mis)[:, :3] * 2.0 - 1.0)
            final_normal = ffnormal.copy()
            pm = nid0 != 0xFFFF
            if pm.any():                                                                            # :206-219
                sign = v[0][pm, 7]
                N = ffnormal[pm]
                Tt = _normalize(tangent_w[pm] - N * (N * tangent_w[pm]).sum(-1, keepdims=True))
                B = _normalize(np.cross(N, Tt)) * sign[:, None]
                TBN = np.stack([Tt, B, N], -1)       # mat3x3f(T, B, N): columns
                if "tbn_transposed" in mis:
                    TBN = TBN.transpose(0, 2, 1)
                final_normal[pm] = _normalize(np.einsum("pij,pj->pi", TBN, normal_local[pm]))
            return matf[:, 0:3] * tex_color[:, :3] * occlusion[:, None], final_normal                # :221

        albedo, final_normal = textured(tex_uv)
        enc = encode_octahedral(final_normal, mis)
        # how far albedo and normal move when uv moves by uv_delta: a texture turns an f32 uv error into a value error this large
        alb_s, nrm_s = np.zeros((len(k), 3)), np.zeros((len(k), 2))
        for d in ((uv_delta, 0.0), (-uv_delta, 0.0), (0.0, uv_delta), (0.0, -uv_delta)):
            a2, n2 = textured(tex_uv + np.array(d))
            alb_s = np.maximum(alb_s, np.abs(a2 - albedo)); nrm_s = np.maximum(nrm_s, np.abs(encode_octahedral(n2, mis) - enc))
        # motion (:230-242)
        ph = np.concatenate([pos, np.ones((len(k), 1))], -1)
        cc = ph @ c["view_proj"].T
        pc = ph @ c["prev_view_proj"].T
        flip = np.array([0.5, 0.5]) if "no_y_flip" in mis else np.array([0.5, -0.5])
        curr_uv = cc[:, :2] / cc[:, 3:4] * flip + 0.5
        prev_uv = pc[:, :2] / pc[:, 3:4] * flip + 0.5
        motion = curr_uv - prev_uv if "motion_sign" in mis else prev_uv - curr_uv
        out["pos"][k] = pos; out["mat_id"][k] = mat_id; out["normal"][k] = final_normal
        out["enc_normal"][k] = enc; out["uv"][k] = tex_uv
        out["albedo_sens"][k] = alb_s; out["normal_sens"][k] = nrm_s
        out["albedo"][k] = albedo; out["motion"][k] = motion
        Tg = sc["tris"][g].astype(np.float64)
        out["cos"][k] = np.abs((_normalize(np.cross(Tg[:, 3:6], Tg[:, 6:9])) * dirs[k]).sum(-1))   # incidence: how a ray's error moves the hit
    # miss (:114-121): pos (0, 0, 0, -1), normal 0, albedo (0, 0, 0, 1), motion 0 — the zero fills above
    return {key: val.reshape((H, W) + val.shape[1:]) for key, val in out.items()}


# ------------------------------------------------------------------------------------------------ post.wgsl main
def _tonemap(c):                                     # :51-53
    return c / (1.0 + c.max(-1, keepdims=True))


def _inverse_tonemap(c):                             # :55-57
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / (1.0 - c.max(-1, keepdims=True))


def _ycocg(c):                                       # :36-41
    return np.stack([c @ [0.25, 0.5, 0.25], c @ [0.5, 0.0, -0.5], c @ [-0.25, 0.5, -0.25]], -1)


def _rgb(c):                                         # :43-48
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([y + co - cg, y + cg, y - co - cg], -1)


def _gauss(x, sigma):                                # :21-26 (every call site has sigma >= 0.001)
    return np.exp(-(x * x) / (2.0 * sigma * sigma))


def _mix(a, b, t):                                   # WGSL mix: a * (1 - t) + b * t
    return a * (1.0 - t) + b * t


def post_f64(inp, W, H, frame_count, jitter=(0.0, 0.0), mis=()):
    """inp: the buffers post reads, as read back: gpos (H, W, 4) f32, gnormal (H, W, 4) f32, galbedo (H, W, 4) u8, raw (H, W, 4) f16,
    motion (H, W, 2) f32, history (H, W, 4) f32. Returns (accum rgb, display rgb before unorm8, final_tm): float64 (H, W, 3) each.
    Pixel and tap positions (uv, prev_uv) are formed in f32 as the shader forms them, because they choose taps and branches; every
    value computed from them is float64."""
    f32 = np.float32
    raw = inp["raw"].astype(np.float64)[..., :3]
    alb = inp["galbedo"].astype(np.float64)[..., :3] / 255.0
    nrm = decode_octahedral(inp["gnormal"][..., :2])
    pos = inp["gpos"].astype(np.float64)[..., :3]
    hist = inp["history"].astype(np.float64)[..., :3]
    ys, xs = np.mgrid[0:H, 0:W]
    uv = (np.stack([xs, ys], -1).astype(f32) + f32(0.5)) / np.array([W, H], f32)                   # :70
    unjitter = np.array([-jitter[0], jitter[1]], f32) * f32(0.5)                                   # :73
    jittered = jitter[0] != 0.0 or jitter[1] != 0.0

    def bilinear(img, cx, cy):
        """textureSampleLevel of the (Rgba16Float / Rgba8Unorm) target at the centre of pixel (cx, cy) + unjitter_offset: Linear, Repeat."""
        if jittered:     # :99-100 as the shader forms them, in f32: the rounding moves the footprint, and the taps may be 65504 apart
            suv = (np.stack([cx, cy], -1).astype(f32) + f32(0.5)) / np.array([W, H], f32) + unjitter.astype(f32)
            x, y = suv[..., 0] * f32(W) - f32(0.5), suv[..., 1] * f32(H) - f32(0.5)
        else:            # the sample point is a texel centre, and the sample the texel itself
            x, y = np.asarray(cx, np.float64), np.asarray(cy, np.float64)
        fx, fy = np.floor(x), np.floor(y)
        ax, ay = (x - fx).astype(np.float64)[..., None], (y - fy).astype(np.float64)[..., None]
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        t = lambda xi, yi: img[np.mod(yi, H), np.mod(xi, W)]
        return (t(x0, y0) * (1 - ax) + t(x0 + 1, y0) * ax) * (1 - ay) + (t(x0, y0 + 1) * (1 - ax) + t(x0 + 1, y0 + 1) * ax) * ay

    center_color = bilinear(raw, xs, ys)                                                            # :77
    center_albedo = bilinear(alb, xs, ys)                                                           # :78
    sum_color = np.zeros((H, W, 3)); sum_weight = np.zeros((H, W))
    for dy in range(-2, 3):                                                                         # :95-136
        for dx in range(-2, 3):
            nx, ny = xs + dx, ys + dy
            inside = (nx >= 0) & (ny >= 0) & (nx < W) & (ny < H)
            cnx, cny = np.clip(nx, 0, W - 1), np.clip(ny, 0, H - 1)
            s_col = bilinear(raw, nx, ny)
            s_alb = bilinear(alb, nx, ny)
            w_spatial = _gauss(np.hypot(dx, dy), 1.5)
            w_color = _gauss(np.linalg.norm(s_alb - center_albedo, axis=-1), 0.2)
            w_normal = np.clip((nrm * nrm[cny, cnx]).sum(-1), 0.0, 1.0) ** 20.0
            w_pos = _gauss(np.linalg.norm(pos[cny, cnx] - pos, axis=-1), 0.1)
            wgt = np.where(inside, w_spatial * w_color * w_normal * w_pos, 0.0)
            sum_color += s_col * wgt[..., None]
            sum_weight += wgt
    with np.errstate(divide="ignore", invalid="ignore"):
        filtered = np.where((sum_weight > 0.001)[..., None], sum_color / sum_weight[..., None], center_color)   # :138-141
    tm_filtered = _tonemap(filtered)                                                                # :148
    m1 = np.zeros((H, W, 3)); m2 = np.zeros((H, W, 3))
    for dy in range(-1, 2):                                                                         # :150-170
        for dx in range(-1, 2):
            nx, ny = xs + dx, ys + dy
            inside = (nx >= 0) & (ny >= 0) & (nx < W) & (ny < H)
            s_col = np.where(inside[..., None], bilinear(raw, nx, ny), filtered)
            s = _ycocg(_tonemap(s_col))
            m1 += s; m2 += s * s
    m1 /= 9.0; m2 /= 9.0
    sigma = np.sqrt(np.maximum(0.0, m2 - m1 * m1))                                                 # :174
    c_min, c_max = m1 - 1.2 * sigma, m1 + 1.2 * sigma
    history_color = tm_filtered.copy()
    valid = np.zeros((H, W), bool)
    motion = np.zeros((H, W, 2))
    if frame_count > 0:                                                                             # :187-229
        mv32 = inp["motion"].astype(f32)
        motion = mv32.astype(np.float64)
        prev_uv = uv + mv32                                                                         # :191, in f32
        valid = (prev_uv[..., 0] >= 0) & (prev_uv[..., 1] >= 0) & (prev_uv[..., 0] <= 1) & (prev_uv[..., 1] <= 1)   # :203
        prev_pos = (prev_uv * np.array([W, H], f32) - f32(0.5)).astype(np.float64)                 # :193, in f32: it picks the taps
        with np.errstate(invalid="ignore"):
            fl = np.floor(np.where(valid[..., None], prev_pos, 0.0))
        f = np.where(valid[..., None], prev_pos, 0.0) - fl                                          # :201 fract
        p0 = fl.astype(np.int64)
        taps = []
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):                                             # :196-199, :219-222
            tx, ty = p0[..., 0] + ox, p0[..., 1] + oy
            ok = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
            v = _tonemap(hist[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)])
            taps.append(v if "history_clamped" in mis else np.where(ok[..., None], v, 0.0))
        c01 = _mix(taps[0], taps[1], f[..., 0:1])
        c23 = _mix(taps[2], taps[3], f[..., 0:1])
        history_color = np.where(valid[..., None], _mix(c01, c23, f[..., 1:2]), history_color)     # :224-227
    final_tm = tm_filtered.copy()
    clamped = _rgb(np.clip(_ycocg(history_color), c_min, c_max))                                   # :236-239
    # speed (:243-244): |motion * size| in f32 as the shader evaluates it, since it only selects a branch (:247) and the smoothstep weight
    m32 = inp["motion"].astype(f32) * np.array([W, H], f32) if frame_count > 0 else np.zeros((H, W, 2), f32)
    speed32 = np.sqrt(m32[..., 0] * m32[..., 0] + m32[..., 1] * m32[..., 1])
    speed = np.hypot(motion[..., 0] * W, motion[..., 1] * H)
    still = (speed32 <= f32(0.5)) if "speed_le" in mis else (speed32 < f32(0.5))
    accum_blend = np.clip(1.0 - 1.0 / (frame_count + 1.0), 0.0, 1.0)                               # :256
    t_s = np.clip(speed / 2.0, 0.0, 1.0)
    feedback = _mix(0.98, 0.85, t_s * t_s * (3.0 - 2.0 * t_s))                                      # :264 smoothstep(0, 2, speed)
    blended = np.where(still[..., None], _mix(tm_filtered, history_color, accum_blend), _mix(tm_filtered, clamped, feedback[..., None]))
    final_tm = np.where(valid[..., None], blended, final_tm)
    final = np.maximum(0.0, _inverse_tonemap(final_tm))                                             # :270-271
    display = final ** (1.0 / 2.2)                                                                  # :279
    return final, display, final_tm
