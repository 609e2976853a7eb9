"""The two reservoir passes — the temporal merge (restir.wgsl main :842-917) and the spatial neighbour loop (restir_spatial.wgsl main :857-993, with
the W clamp of :1001-1012) — against their float64 restatement (tests/_wgsl_f64_restir.py) on crafted inputs written through the existing ABI.
A real scene is advanced to frame fc and its G-buffer rendered; the buffers the pass reads are overwritten through write_rows with data that reaches
every branch (craft_temporal / craft_spatial), the one phase runs, and both what it read and what it wrote are read back: float64 is handed the bytes
read back. Runs on the oracle and on the product's host-compiled stage functions (CPU suite) and on libfrt.so (-m gpu, where the kernels must also
equal the oracle bit for bit). Slots, proven by read-back in run_*: in the middle of frame fc the G-buffer of the frame is index fc & 1, the previous
frame's the other one, motion and the candidate record index 0, reservoirs[0] the temporal and [1] the spatial result.

Exact outside the ambiguous mask: M, y, which s_path was kept (bit for bit against its source), the zero reservoir on background pixels. Bounded:
w_sum, p_hat, W, by the per-pixel bounds derived in _wgsl_f64_restir.py (rounding counts times 2^-24 times the pixel's conditioning)."""
import numpy as np
import pytest
import _wgsl_f64_restir as R

GPOS, GNORMAL, GALBEDO, GMOTION, RESERVOIR, RAW, CANDIDATE = 0, 1, 2, 3, 4, 5, 8
SIZES = [(1, 1), (9, 1), (2, 3), (17, 16), (64, 48), (200, 120)]
FRAMES = [0, 1, 5, 5000]              # 5000 * 927163 and 5000 * 0x12345678 wrap u32
MAX_AMBIGUOUS = 0.02                  # share of pixels float64 may leave undecided, per case (a condition on the inputs, not a tolerance)
ORACLE_SHARE = 0.5                    # the f32 reading of the reference must stay within half of the derived worst-case bounds wherever a bound
LONG_CHAIN = 8                        # counts at least this many roundings. Shorter chains reach their worst case for real: the 20 / M rescale is two or
                                      # three roundings, and two roundings of up to 2^-24 each add up to more than half of 3 * 2^-24 a quarter of the time
                                      # (measured: 0.50 of its bound); nothing is widened for them, they are only not held to the half.
f32 = np.float32


# ------------------------------------------------------------------------------------------------ scenes
def probe_scene(frt, orc):
    """Cornell walls, a diffuse and a mirror box, a glass sphere — and materials specular by exactly one clause of restir.wgsl:870 each, between the
    limits of the validity test (0.2 / 0.8 / 0.01) and of the narrow search (0.1 / 0.9 / 0.1), which no named scene holds. Material 0 is diffuse."""
    import _scenes as S
    b = S.DualBuilder(frt, orc)
    plane, cube, sph = (b.add_mesh(*S._geo(frt, "create_plane")), b.add_mesh(*S._geo(frt, "create_cube")), b.add_mesh(*S._geo(frt, "create_sphere", 2)))

    def mat(rgb, rough=0.5, metal=0.0, trans=0.0):
        m = frt.material_new(list(rgb) + [1.0]); m.roughness = rough; m.metallic = metal; m.transmission = trans; m.ior = 1.5
        return b.add_material(m)
    white, red, green = mat((0.73, 0.73, 0.73)), mat((0.65, 0.05, 0.05)), mat((0.12, 0.45, 0.15))
    mirror, glass = mat((0.8, 0.8, 0.8), 0.01, 1.0), mat((0.5, 0.8, 1.0), 0.0, 0.0, 1.0)
    lm = b.add_material(S._emissive(frt, 0, (1, 1, 1), 10.0))
    mat((0.6, 0.6, 0.6), 0.15); mat((0.6, 0.5, 0.4), 0.5, 0.85); mat((0.4, 0.5, 0.6), 0.5, 0.0, 0.05); mat((0.7, 0.7, 0.7), 0.05)
    ref = frt.scenes.create_cornell_box().get("instances")
    for k, m in ((0, white), (1, white), (2, white), (3, red), (4, green)):
        b.add_instance(plane, m, ref[k, 5:21].view(f32))
    b.add_instance(plane, lm, ref[5, 5:21].view(f32))
    b.add_light(S._quad_light(frt, (0, 0.99, 0), 0.25, (1, 1, 1, 10)))
    b.add_instance(cube, white, S._mat(-0.35, -0.4, -0.3, 0.5, 1.2, 0.5))
    b.add_instance(cube, mirror, S._mat(0.4, -0.7, 0.2, 0.5, 0.6, 0.5))
    b.add_instance(sph, glass, S._mat(0.0, -0.2, 0.45, 0.4, 0.4, 0.4))
    return b.build()


def named_scene(frt, orc, which):
    fs, os_ = (frt.scenes.create_cornell_box(), orc.cornell()) if which == "cornell" else (frt.scenes.create_restir_scene(), orc.restir_scene())
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    return fs, os_


_SCENES = {}


def scene(frt, orc, which):
    if which not in _SCENES:
        _SCENES[which] = probe_scene(frt, orc) if which == "probe" else named_scene(frt, orc, which)
    return _SCENES[which]


def material_classes(materials):
    """Material ids by how restir.wgsl:870 / restir_spatial.wgsl:792, :906 see them (None: the scene has none)."""
    m = materials.view(f32)
    r, me, t = m[:, 7], m[:, 8], m[:, 9]
    first = lambda k: int(np.nonzero(k)[0][0]) if k.any() else None
    return {"diffuse": first((r >= f32(0.2)) & (me <= f32(0.8)) & (t <= f32(0.01))),
            "rough_only": first((r < f32(0.2)) & (me <= f32(0.8)) & (t <= f32(0.01))), "metal_only": first((r >= f32(0.2)) & (me > f32(0.8)) & (t <= f32(0.01))),
            "trans_only": first((r >= f32(0.2)) & (me <= f32(0.8)) & (t > f32(0.01))),
            "narrow": first((r < f32(0.1)) | (me > f32(0.9)) | (t > f32(0.1)))}


# ------------------------------------------------------------------------------------------------ crafting helpers
def encode_oct(n):
    """Unit vectors -> octahedral pair in f32 (any encoding will do: the passes decode what is stored, and so does float64)."""
    n = n / np.abs(n).sum(-1, keepdims=True)
    x, y = n[..., 0], n[..., 1]
    sx, sy = np.where(x >= 0, 1.0, -1.0), np.where(y >= 0, 1.0, -1.0)
    fold = np.stack([(1 - np.abs(y)) * sx, (1 - np.abs(x)) * sy], -1)
    return np.where((n[..., 2] < 0)[..., None], fold, n[..., :2]).astype(f32)


def tilt(n, cosine, rng):
    """Unit vectors at the given cosine to n, in a random direction."""
    a = rng.normal(size=n.shape)
    t = a - n * (a * n).sum(-1, keepdims=True)
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    return n * cosine + t * np.sqrt(1 - cosine * cosine)


def random_reservoirs(rng, n, lo=-1.0, hi=1.0):
    r = np.zeros(n, R.RES)
    r["y"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    r["M"] = rng.integers(2, 31, n); r["W"] = rng.uniform(0.05, 3.0, n); r["p_hat"] = rng.uniform(0.01, 2.0, n)
    r["s"] = rng.uniform(lo, hi, (n, 3)); r["w_sum"] = r["p_hat"] * r["W"] * r["M"]
    return r


def craft_temporal(W, H, gpos, gnormal, galbedo, materials, view_pos, seed):
    """Everything restir.wgsl:846-917 reads, reaching every branch. Positions and normals stay finite and pos.w a valid material index or -1:
    T-trace traces real rays from the current G-buffer. Non-finite values only in motion."""
    rng = np.random.default_rng(seed)
    n = W * H
    cls = material_classes(materials)
    gp, gn, ga = gpos.reshape(n, 4).copy(), gnormal.reshape(n, 4).copy(), galbedo.reshape(n, 4).copy()
    surf = gp[:, 3] >= 0
    pick = lambda k, p: surf & (rng.random(n) < p) if k is not None else np.zeros(n, bool)
    for name, p in (("rough_only", 0.05), ("metal_only", 0.05), ("trans_only", 0.05), ("narrow", 0.03)):       # specular by each clause of :870
        m = pick(cls[name], p); gp[m, 3] = f32(cls[name] or 0)
    near = surf & (rng.random(n) < 0.08)                             # within 0.1 of the camera: the 1e-5 arm of max(1e-5, 0.001 d^2)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    gp[near, :3] = (np.asarray(view_pos[:3], np.float64) + d[near] * rng.uniform(0.02, 0.06, (near.sum(), 1))).astype(f32)
    # x == W through prev_uv.x == 1 with zeros that pass the validity test (material 0, normal +z, position 0, black): the texel reads give zeros, the
    # storage buffer is indexed linearly (:855)
    lin = np.zeros(n, bool); lin[0:n:W] = rng.random(len(range(0, n, W))) < 0.5
    if cls["diffuse"] == 0:
        gp[lin] = 0; gn[lin] = 0; ga[lin] = (0, 0, 0, 255)
    else:
        lin[:] = False
    pp, pn, pa = gp.copy(), gn.copy(), ga.copy()                     # previous frame: the same surface, then one change per pixel
    nrm = R.decode_octahedral(gn[:, :2])
    case = rng.integers(0, 14, n)
    pp[case == 4] = (0, 0, 0, -1)                                    # reprojection onto a background pixel
    m = (case == 5) & surf; pp[m, 3] = np.where(pp[m, 3] == 0, f32(1), f32(0))     # another material
    for c, cosine in ((6, 0.99 + 1e-3), (7, 0.99 - 1e-3)):           # the normal on either side of 0.99
        m = case == c; pn[m, :2] = encode_oct(tilt(nrm[m], cosine, rng))
    thr = np.maximum(1e-5, ((gp[:, :3].astype(np.float64) - np.asarray(view_pos[:3], np.float64)) ** 2).sum(-1) * 0.001)
    for c, k in ((8, 0.9), (9, 1.1), (10, 1e-3), (11, 30.0)):        # the position on either side of the threshold, on both arms (near / not)
        m = case == c; pp[m, :3] = (gp[m, :3].astype(np.float64) + d[m] * np.sqrt(thr[m] * k)[:, None]).astype(f32)
    ac = rng.integers(0, 12, n)                                      # (l_curr + 0.001) / (l_prev + 0.001) around 3.0 and 0.33; black
    for c, (a_cur, a_prev) in ((4, (90, 30)), (5, (91, 30)), (6, (30, 90)), (7, (29, 90)), (8, (0, 0)), (9, (120, 0)), (10, (0, 120))):
        m = (ac == c) & ~lin; ga[m, :3] = a_cur; pa[m, :3] = a_prev
    ys, xs = np.divmod(np.arange(n), W)
    size = np.array([W, H], f32)
    uv = (np.stack([xs, ys], -1).astype(f32) + f32(0.5)) / size
    mot = np.zeros((n, 2), f32)
    mc = rng.integers(0, 14, n)
    m = mc == 6; mot[m] = -uv[m]                                     # prev_uv exactly 0
    m = mc == 7; mot[m] = f32(1) - uv[m]                             # prev_uv 1: the texel index equals the size
    m = mc == 8; mot[m] = (1.5, -0.25)                               # outside
    m = mc == 9; mot[m] = np.nan
    m = mc >= 10; mot[m] = (rng.integers(-3, 4, (m.sum(), 2)) / size).astype(f32)     # onto other pixels, some off the image
    mot[lin] = np.stack([f32(1) - uv[lin, 0], np.zeros(lin.sum(), f32)], -1)
    prev = random_reservoirs(rng, n)
    prev["M"] = rng.choice(np.array([0, 1, 15, 16, 17, 2 ** 31, 7, 12, 25], np.uint32), n, p=[.06, .1, .1, .1, .1, .06, .16, .16, .16])
    prev["p_hat"] = np.where(rng.random(n) < 0.8, prev["p_hat"], rng.choice(np.array([0, 1e-30, 1e30], f32), n))
    k = rng.random(n); prev["W"] = np.where(k < 0.1, f32(0), np.where(k < 0.2, f32(20), prev["W"] * f32(0.1)))
    other = random_reservoirs(rng, n)                                # buffers[0] before the pass: the temporal pass must not read it
    cand = np.zeros((n, 4), f32)                                     # a fully crafted candidate, for the host probe (the renderers trace their own)
    cand[:, :3] = rng.uniform(-1, 1, (n, 3)); cand[:, 3] = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.0, 1.5, n))
    sh = lambda a, c: a.reshape(H, W, c)
    return {"gpos": sh(gp, 4), "gnormal": sh(gn, 4), "galbedo": sh(ga, 4), "gpos_prev": sh(pp, 4), "gnormal_prev": sh(pn, 4), "galbedo_prev": sh(pa, 4),
            "motion": sh(mot, 2), "prev_res": prev.reshape(H, W), "temporal_res": other.reshape(H, W), "cand": sh(cand, 4)}


def craft_spatial(W, H, gpos, gnormal, galbedo, res, materials, view_pos, seed):
    """The real G-buffer and temporal reservoirs of a rendered frame for most pixels; a share perturbed to straddle each validity threshold on the
    diffuse and the specular arm, crafted centre M, p_hat <= 0, W, albedo pairs and s_path cases (restir_spatial.wgsl:893-992)."""
    rng = np.random.default_rng(seed)
    n = W * H
    cls = material_classes(materials)
    gp, gn, ga = gpos.reshape(n, 4).copy(), gnormal.reshape(n, 4).copy(), galbedo.reshape(n, 4).copy()
    rs = res.reshape(n).copy()
    surf = gp[:, 3] >= 0
    ys, xs = np.divmod(np.arange(n), W)
    # tiles of one crafted material, so that neighbours share it: specular by one clause each, and the narrow search
    tile = (ys // 6) * ((W + 5) // 6) + xs // 6
    ids = [cls[k] for k in ("rough_only", "metal_only", "trans_only", "narrow") if cls[k] is not None]
    spec_tile = np.zeros(n, bool)
    if ids:
        choice = rng.integers(0, 4 * len(ids), tile.max() + 1)       # a quarter of the tiles
        spec_tile = surf & (choice[tile] < len(ids))
        gp[spec_tile, 3] = np.asarray(ids, f32)[choice[tile][spec_tile]]
        # the specular arm accepts neighbours within 0.01: gather the tile's pixels around its first surface pixel, on either side of that distance
        firsts = {}
        for i in np.nonzero(spec_tile)[0]:
            firsts.setdefault(tile[i], i)
        base = np.array([firsts.get(t, 0) for t in tile])
        gp[spec_tile, :3] = gp[base[spec_tile], :3] + rng.uniform(-0.0045, 0.0045, (spec_tile.sum(), 3)).astype(f32)
        gn[spec_tile] = gn[base[spec_tile]]
    nrm = R.decode_octahedral(gn[:, :2])
    case = rng.integers(0, 24, n)
    for c, cosine in ((10, 0.995 + 1e-3), (11, 0.995 - 1e-3), (12, 0.998 + 1e-3), (13, 0.998 - 1e-3)):
        m = (case == c) & surf; gn[m, :2] = encode_oct(tilt(nrm[m], cosine, rng))
    thr = np.maximum(1e-5, ((gp[:, :3].astype(np.float64) - np.asarray(view_pos[:3], np.float64)) ** 2).sum(-1) * 0.001)
    for c, k in ((14, 0.9), (15, 1.1)):                              # off the surface by either side of the diffuse arm's threshold
        m = (case == c) & surf & ~spec_tile; gp[m, :3] = (gp[m, :3].astype(np.float64) + nrm[m] * np.sqrt(thr[m] * k)[:, None]).astype(f32)
    gp[case == 16] = (0, 0, 0, -1); gn[case == 16] = 0
    surf = gp[:, 3] >= 0
    grey = rng.choice(np.array([0, 3, 25, 39, 40, 80, 255], np.uint8), n)           # Jacobian to both clamp ends; around 0.5 and 2.0 (80 / 40, 80 / 39)
    m = rng.random(n) < 0.3; ga[m, :3] = grey[m, None]
    # reservoirs
    pos, nn = gp[:, :3].astype(np.float64), R.decode_octahedral(gn[:, :2])
    m = rng.random(n) < 0.25                                         # the centre's 20 / M rescale
    rs["M"][m] = rng.choice(np.array([0, 19, 20, 21, 1000], np.uint32), m.sum())
    rs["w_sum"][m] = np.where(rs["M"][m] == 0, 0.0, rng.uniform(0.0, 40.0, m.sum()))
    m = rng.random(n) < 0.1; rs["p_hat"][m] = rng.choice(np.array([0.0, -1.0], f32), m.sum())
    k = rng.random(n); rs["W"] = np.where(k < 0.08, f32(0), np.where(k < 0.12, f32(20), rs["W"]))
    m = rng.random(n) < 0.15; rs["M"][m] = rng.integers(1, 40, m.sum()); rs["W"][m] = rng.uniform(0.1, 3.0, m.sum()); rs["p_hat"][m] = rng.uniform(0.01, 2.0, m.sum())
    m = rng.random(n) < 0.2; rs["y"][m] = rng.integers(0, 2 ** 32, m.sum(), dtype=np.uint64).astype(np.uint32)
    sc = rng.integers(0, 16, n)                                      # s_path: 0-7 as the temporal stage left it
    t = tilt(nn, 0.0, rng)
    hemi = tilt(nn, 0.7, rng)
    tw = (-1.0 - pos[:, 2]) / np.minimum(hemi[:, 2], -1e-9)          # just behind the back wall (the plane z = -1 of every scene used here): the wall
    hitp = pos + hemi * tw[:, None]                                  # then lies inside (0.999 dist, dist), visible only because t_max is 0.999 dist
    m = (sc == 8) & (hemi[:, 2] < -0.3) & (np.abs(hitp[:, :2]) < 0.95).all(-1) & (tw > 0.05); rs["s"][m] = pos[m] + hemi[m] * (tw[m] * 1.0005)[:, None]
    m = sc == 9; rs["s"][m] = pos[m] - nn[m] * 0.3 + t[m] * 0.1                     # behind the surface
    m = sc == 10; rs["s"][m] = pos[m] + nn[m] * 0.0005                              # closer than 0.001
    m = sc == 11; rs["s"][m] = pos[m] + hemi[m] * 6.0                               # beyond the walls: occluded (or out through the open front)
    m = sc == 12; rs["s"][m] = (-0.35, -0.4, -0.3)                                  # inside the tall box: occluded
    m = sc == 13; rs["s"][m] = pos[m] + t[m] * 0.5 + nn[m] * (0.5 * rng.choice([0.0005, 0.0015, 0.003, 0.02], m.sum()))[:, None]   # grazing: cos_neigh around 0.001
    m = sc == 14; rs["s"][m] = gp[m, :3]                                            # the neighbour's own position
    m = sc == 15; rs["s"][m] = pos[m] + hemi[m] * rng.uniform(0.002, 0.3, (m.sum(), 1))   # close and visible
    rs["s"][~np.isfinite(rs["s"]).all(-1)] = 0
    rs[~surf] = np.zeros(1, R.RES)
    sh = lambda a, c: a.reshape(H, W, c)
    return {"gpos": sh(gp, 4), "gnormal": sh(gn, 4), "galbedo": sh(ga, 4), "in_res": rs.reshape(H, W)}


# ------------------------------------------------------------------------------------------------ running one phase
class IO:
    """read / write / phases / end_frame of either renderer."""

    def __init__(self, r, H, cam, oracle):
        self.read = (lambda b, i=0: r.read(b, i)) if oracle else (lambda b, i=0: r.read_buffer(b, i))
        self.write = lambda b, i, d: r.write_rows(b, i, 0, H, np.ascontiguousarray(d).view(np.uint8))
        self.phases = (lambda p: r.render_phases(cam, p, 0, H)) if oracle else (lambda p: r.render_phases(cam, p))
        self.end_frame = r.end_frame


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_temporal(io, W, H, fc, materials, view_pos, seed, offscreen=False):
    """Advance to frame fc, render its G-buffer, overwrite what the temporal stage reads, run TEMPORAL alone. offscreen: every motion vector points off
    the image, so that the stored reservoir is the fresh candidate (:833-840, :907-917). Returns (inputs as read back, stored reservoirs)."""
    for _ in range(fc):
        io.end_frame()
    io.phases(1)
    cur, prv = fc & 1, (fc & 1) ^ 1
    c = craft_temporal(W, H, io.read(GPOS, cur).view(f32), io.read(GNORMAL, cur).view(f32), io.read(GALBEDO, cur), materials, view_pos, seed)
    if offscreen:
        c["motion"] = np.full((H, W, 2), 5.0, f32)
    for buf, key in ((GPOS, "gpos"), (GNORMAL, "gnormal"), (GALBEDO, "galbedo")):
        io.write(buf, cur, c[key]); io.write(buf, prv, c[key + "_prev"])
    io.write(GMOTION, 0, c["motion"]); io.write(RESERVOIR, 1, c["prev_res"]); io.write(RESERVOIR, 0, c["temporal_res"])
    io.phases(2)
    inp = {"gpos": io.read(GPOS, cur).view(f32), "gnormal": io.read(GNORMAL, cur).view(f32), "galbedo": io.read(GALBEDO, cur),
           "gpos_prev": io.read(GPOS, prv).view(f32), "gnormal_prev": io.read(GNORMAL, prv).view(f32), "galbedo_prev": io.read(GALBEDO, prv),
           "motion": io.read(GMOTION, 0).view(f32), "prev_res": io.read(RESERVOIR, 1).view(R.RES).reshape(H, W), "temporal_res": c["temporal_res"]}
    # the slot rule: the stage read G-buffer slot fc & 1 as current and the other as previous, motion 0, reservoirs[1]; it wrote reservoirs[0]
    for k in ("gpos", "gnormal", "galbedo", "gpos_prev", "gnormal_prev", "galbedo_prev", "motion", "prev_res"):
        assert _same(inp[k], c[k]), f"{k}: the bytes read back are not the bytes written"
    out = io.read(RESERVOIR, 0).view(R.RES).reshape(H, W)
    assert not _same(out, c["temporal_res"]), "the temporal stage did not write reservoirs[0]"
    return inp, out


def run_spatial(io, W, H, fc, materials, view_pos, seed):
    """Advance to frame fc, render G-buffer and temporal stage, overwrite what the spatial stage reads, run SPATIAL alone."""
    for _ in range(fc):
        io.end_frame()
    io.phases(1 | 2)
    cur = fc & 1
    c = craft_spatial(W, H, io.read(GPOS, cur).view(f32), io.read(GNORMAL, cur).view(f32), io.read(GALBEDO, cur),
                      io.read(RESERVOIR, 0).view(R.RES).reshape(H, W), materials, view_pos, seed)
    junk = random_reservoirs(np.random.default_rng(seed + 1), W * H).reshape(H, W)
    for buf, key in ((GPOS, "gpos"), (GNORMAL, "gnormal"), (GALBEDO, "galbedo")):
        io.write(buf, cur, c[key])
    io.write(RESERVOIR, 0, c["in_res"]); io.write(RESERVOIR, 1, junk)
    io.phases(4)
    inp = {"gpos": io.read(GPOS, cur).view(f32), "gnormal": io.read(GNORMAL, cur).view(f32), "galbedo": io.read(GALBEDO, cur),
           "in_res": io.read(RESERVOIR, 0).view(R.RES).reshape(H, W)}
    for k in inp:
        assert _same(inp[k], c[k]), f"{k}: the bytes read back are not the bytes written"
    out = io.read(RESERVOIR, 1).view(R.RES).reshape(H, W)
    assert not _same(out, junk), "the spatial stage did not write reservoirs[1]"
    return inp, out, io.read(RAW, 0).view(np.float16)


# ------------------------------------------------------------------------------------------------ comparisons
def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check_temporal(inp, out, W, H, fc, view_pos, materials, mis=()):
    """Stored reservoirs against float64. Returns ((worst residual / bound, the same over bounds of at least LONG_CHAIN roundings), ambiguous share, pixels merged)."""
    ref = R.temporal_merge_f64(inp, W, H, fc, view_pos, materials, mis)
    zero3 = np.zeros((H, W, 3), np.uint32)
    prev_s = _bits(inp["prev_res"]["s"]).reshape(H * W, 3)[np.maximum(ref["prev_index"], 0).reshape(-1)].reshape(H, W, 3)
    if "other_reservoirs" in mis:
        prev_s = _bits(inp["temporal_res"]["s"]).reshape(H * W, 3)[np.maximum(ref["prev_index"], 0).reshape(-1)].reshape(H, W, 3)
    cand_s = _bits(inp["cand"][..., :3])
    got = {k: out[k].astype(np.float64) for k in ("w_sum", "W", "p_hat")}

    def matches(pre):
        sel = ref[pre + "sel"]
        want_s = np.where((sel == 1)[..., None], cand_s, np.where((sel == 2)[..., None], prev_s, zero3))
        ok = (out["M"].astype(np.int64) == ref["M"]) & (out["y"].astype(np.int64) == ref[pre + "y"].astype(np.int64)) & (_bits(out["s"]) == want_s).all(-1)
        worst = np.zeros((H, W)); long_ = np.zeros((H, W))
        for k, rk in (("w_sum", "w_sum"), ("p_hat", pre + "p_hat"), ("W", pre + "W")):
            tol = ref[rk + "_tol"]
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.abs(got[k] - ref[rk])
                ok &= d <= tol
                sh_k = np.where(tol > 0, d / np.where(tol > 0, tol, 1), 0.0)
                worst = np.maximum(worst, sh_k)
                long_ = np.maximum(long_, np.where(tol >= LONG_CHAIN * R.EPS * np.abs(ref[rk]), sh_k, 0.0))
        return ok, worst, long_
    ok, worst, long_ = matches("")
    ok2, worst2, long2 = matches("alt_")
    passed = ok | (ref["ris_amb"] & ok2)                             # the RIS draw alone undecided: either float64 outcome
    worst = np.where(ok, worst, worst2); long_ = np.where(ok, long_, long2)
    judged = ~ref["ambiguous"]
    bad = judged & ~passed
    assert not bad.any(), (f"temporal: {int(bad.sum())} pixels differ from float64, first at {tuple(np.argwhere(bad)[0])}: got "
                           f"{out[tuple(np.argwhere(bad)[0])]}, want " + str({k: ref[k][tuple(np.argwhere(bad)[0])] for k in ("y", "M", "w_sum", "W", "p_hat", "sel")}))
    amb = float((ref["ambiguous"] | ref["ris_amb"]).mean())
    assert amb <= MAX_AMBIGUOUS, f"temporal: float64 leaves {amb:.2%} of the pixels undecided"
    return (float(np.where(judged & passed, worst, 0.0).max()), float(np.where(judged & passed, long_, 0.0).max())), amb, int(ref["merged"].sum())


def check_spatial(inp, out, raw, W, H, fc, view_pos, materials, tris, mis=(), loop_only=False):
    """Reservoirs after the spatial stage against float64: y, M and w_sum are those the neighbour loop left. loop_only: `out` is the loop's reservoir
    itself (the host probe), without the stage's tail. Returns ((worst residual / bound, the same over bounds of at least LONG_CHAIN roundings), ambiguous share, neighbours merged)."""
    ref = R.spatial_reuse_f64(inp, W, H, fc, view_pos, materials, tris, mis)
    judged = ~ref["ambiguous"]
    w = out["w_sum"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(w - ref["w_sum"])
        ok = (out["M"].astype(np.int64) == ref["M"]) & (out["y"].astype(np.int64) == ref["y"].astype(np.int64)) & (d <= ref["w_sum_tol"])
    bg = ref["background"]
    ok &= ~bg | (np.ascontiguousarray(out).view(np.uint32).reshape(H, W, 8) == 0).all(-1)             # :876-881
    bad = judged & ~ok
    assert not bad.any(), (f"spatial: {int(bad.sum())} pixels differ from float64, first at {tuple(np.argwhere(bad)[0])}: got {out[tuple(np.argwhere(bad)[0])]}, "
                           f"want " + str({k: ref[k][tuple(np.argwhere(bad)[0])] for k in ("y", "M", "w_sum", "w_sum_tol", "merges")}))
    amb = float(ref["ambiguous"].mean())
    assert amb <= MAX_AMBIGUOUS, f"spatial: float64 leaves {amb:.2%} of the pixels undecided"
    if not loop_only and not mis:
        # what float64 cannot predict (trace_path's radiance) is still consistent, from the outputs alone, on EVERY pixel (:1001-1015)
        p, Wo, M = out["p_hat"].astype(np.float64), out["W"].astype(np.float64), out["M"].astype(np.float64)
        assert (raw[bg].astype(np.float64) == 0).all(), "background radiance is not zero"
        assert ((Wo == 0) | (p > 0)).all() and (p >= 0).all(), "W != 0 with p_hat == 0"
        live = (p > 0) & (M > 0) & ~bg
        with np.errstate(divide="ignore", invalid="ignore"):
            want_W = np.clip((1.0 / p) * (w / M), 0.0, 20.0)
            okW = np.abs(Wo - want_W) <= 6 * R.EPS * want_W                                           # 1 / p (2), w_sum / M (2), product (1), +1
        assert okW[live].all(), f"W_out != clamp((1 / p_hat) * (w_sum / M), 0, 20) at {tuple(np.argwhere(live & ~okW)[0])}"
        rgb = raw[..., :3].astype(np.float64)
        fin = np.isfinite(rgb).all(-1) & ~bg
        lum = R.luminance(rgb)
        okL = np.abs(lum - p * Wo) <= 2.0 ** -10 * p * Wo + 2e-7      # f16: 2^-11 per channel (and its subnormal step); the f32 roundings are far below
        assert okL[fin].all(), f"luminance(raw) != p_hat * W at {tuple(np.argwhere(fin & ~okL)[0])}"
        assert (raw[..., 3][~bg].astype(np.float64) == 1).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(judged & (ref["w_sum_tol"] > 0), d / np.where(ref["w_sum_tol"] > 0, ref["w_sum_tol"], 1), 0.0)
    long_ = np.where(ref["w_sum_tol"] >= LONG_CHAIN * R.EPS * np.abs(ref["w_sum"]), share, 0.0)
    return (float(share.max()), float(long_.max())), amb, int(ref["merges"].sum())


# ------------------------------------------------------------------------------------------------ cases
def _cases():
    out = [("probe", W, H, FRAMES[i % 4]) for i, (W, H) in enumerate(SIZES)]
    out += [("probe", 17, 16, fc) for fc in FRAMES if ("probe", 17, 16, fc) not in out]
    out += [("cornell", 64, 48, 1), ("restir", 17, 16, 5)]
    return out


CASES = _cases()
IDS = [f"{s}-{W}x{H}-f{fc}" for s, W, H, fc in CASES]
_ORACLE = {}


def _setup(frt, orc, which, W, H, fc):
    fs, os_ = scene(frt, orc, which)
    cam = frt.CameraController().build_uniform(W / H, fc, fs.num_lights)
    view_pos = np.frombuffer(bytes(cam), f32)[48:52].astype(np.float64)
    return fs, os_, cam, view_pos, fs.get("materials")


def oracle_temporal(frt, orc, which, W, H, fc):
    """The oracle runs the stage fused and has no candidate buffer: a second renderer — same scene, camera, frame count and crafted G-buffer, every
    motion vector off the image — stores the fresh candidate; the first runs the crafted motion."""
    key = ("t", which, W, H, fc)
    if key not in _ORACLE:
        fs, os_, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
        seed = 7000 * W + 13 * H + fc
        ra, rb = os_.renderer(W, H, 1, True, 8), os_.renderer(W, H, 1, True, 8)
        _, fresh = run_temporal(IO(ra, H, cam, True), W, H, fc, mats, view_pos, seed, offscreen=True)
        inp, out = run_temporal(IO(rb, H, cam, True), W, H, fc, mats, view_pos, seed)
        surf = inp["gpos"][..., 3] >= 0
        assert (fresh["M"][surf] == 1).all() and (fresh["M"][~surf] == 0).all(), "the off-image pass did not store the fresh candidate"
        inp["cand"] = np.concatenate([fresh["s"], fresh["p_hat"][..., None]], -1).astype(f32)
        _ORACLE[key] = (inp, out)
    return _ORACLE[key]


def oracle_spatial(frt, orc, which, W, H, fc):
    key = ("s", which, W, H, fc)
    if key not in _ORACLE:
        fs, os_, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
        _ORACLE[key] = run_spatial(IO(os_.renderer(W, H, 1, True, 8), H, cam, True), W, H, fc, mats, view_pos, 9000 * W + 17 * H + fc)
    return _ORACLE[key]


_TRIS = {}


def tris_of(fs, which):
    if which not in _TRIS:
        _TRIS[which] = fs.get("tris")
    return _TRIS[which]


@pytest.mark.parametrize("which,W,H,fc", CASES, ids=IDS)
def test_oracle_temporal_merge_matches_float64(frt, orc, which, W, H, fc):
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    inp, out = oracle_temporal(frt, orc, which, W, H, fc)
    worst, amb, merged = check_temporal(inp, out, W, H, fc, view_pos, mats)
    print(f" temporal {which} {W}x{H} f{fc}: worst residual / bound {worst[0]:.3f} (long chains {worst[1]:.3f}); ambiguous {amb:.3%}; {merged} of {W * H} pixels merged history")
    assert worst[1] <= ORACLE_SHARE, "the f32 reading uses more than half of the derived bound: the derivation (or the reading) is off"


@pytest.mark.parametrize("which,W,H,fc", CASES, ids=IDS)
def test_oracle_spatial_reuse_matches_float64(frt, orc, which, W, H, fc):
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    inp, out, raw = oracle_spatial(frt, orc, which, W, H, fc)
    worst, amb, merges = check_spatial(inp, out, raw, W, H, fc, view_pos, mats, tris_of(fs, which))
    print(f" spatial {which} {W}x{H} f{fc}: worst residual / bound {worst[0]:.3f} (long chains {worst[1]:.3f}); ambiguous {amb:.3%}; {merges} neighbours merged")
    assert worst[1] <= ORACLE_SHARE, "the f32 reading uses more than half of the derived bound: the derivation (or the reading) is off"


def test_crafted_inputs_reach_every_branch(frt, orc):
    """The committed inputs are not tame: on the probe scene at 200x120 every class of decision is taken both ways by a fair number of pixels."""
    which, W, H, fc = "probe", 200, 120, 1
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    cls = material_classes(mats)
    assert all(v is not None for v in cls.values()) and cls["diffuse"] == 0, cls
    inp, out = oracle_temporal(frt, orc, which, W, H, fc)
    ref = R.temporal_merge_f64(inp, W, H, fc, view_pos, mats)
    sel = ref["sel"]
    assert ref["merged"].sum() > W * H // 20 and (sel == 2).sum() > 200 and ((sel == 1) & ref["merged"]).sum() > 200 and (sel == 0).sum() > 0
    lin = (ref["prev_index"] >= 0) & ref["merged"] & (inp["gpos"][..., :3] == 0).all(-1)
    print(f" temporal: {int(ref['merged'].sum())} merges, {int((sel == 2).sum())} kept the history, {int(lin.sum())} read reservoirs through x == W")
    inp, out, raw = oracle_spatial(frt, orc, which, W, H, fc)
    ref = R.spatial_reuse_f64(inp, W, H, fc, view_pos, mats, tris_of(fs, which))
    assert ref["merges"].sum() > W * H // 10 and (ref["narrow"] & (ref["merges"] > 0)).sum() > 20
    assert (out["y"] != inp["in_res"]["y"]).sum() > 500


# ------------------------------------------------------------------------------------------------ the product's host-compiled stage functions
@pytest.mark.parametrize("which,W,H,fc", CASES, ids=IDS)
def test_host_stage_functions_match_float64(frt, orc, hostcheck, which, W, H, fc):
    """temporal_merge_pixel (with a fully crafted candidate) and the neighbour loop of spatial_neighbors, compiled for the host, on the inputs the
    oracle cases read back."""
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    cur, prv = fc & 1, (fc & 1) ^ 1
    rh = hostcheck.renderer(fs, W, H, 1, 1)
    inp, _ = oracle_temporal(frt, orc, which, W, H, fc)
    inp = dict(inp)
    inp["cand"] = craft_temporal(W, H, inp["gpos"], inp["gnormal"], inp["galbedo"], mats, view_pos, 7000 * W + 13 * H + fc)["cand"]
    for buf, key in ((GPOS, "gpos"), (GNORMAL, "gnormal"), (GALBEDO, "galbedo")):
        rh.write(buf, cur, inp[key]); rh.write(buf, prv, inp[key + "_prev"])
    rh.write(GMOTION, 0, inp["motion"]); rh.write(RESERVOIR, 1, inp["prev_res"]); rh.write(RESERVOIR, 0, inp["temporal_res"]); rh.write(CANDIDATE, 0, inp["cand"])
    rh.temporal_merge(cam, fc)
    worst_t, amb_t, merged = check_temporal(inp, rh.read(RESERVOIR, 0).view(R.RES).reshape(H, W), W, H, fc, view_pos, mats)
    sinp, _, _ = oracle_spatial(frt, orc, which, W, H, fc)
    for buf, key in ((GPOS, "gpos"), (GNORMAL, "gnormal"), (GALBEDO, "galbedo")):
        rh.write(buf, cur, sinp[key])
    rh.write(RESERVOIR, 0, sinp["in_res"])
    loop = rh.spatial_neighbors(cam, fc).view(R.RES).reshape(H, W)
    worst_s, amb_s, merges = check_spatial(sinp, loop, None, W, H, fc, view_pos, mats, tris_of(fs, which), loop_only=True)
    print(f" host functions {which} {W}x{H} f{fc}: worst residual / bound temporal {worst_t[0]:.3f}, spatial {worst_s[0]:.3f}; ambiguous {amb_t:.3%} / {amb_s:.3%}")


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


@pytest.mark.gpu
@pytest.mark.parametrize("which,W,H,fc", CASES, ids=IDS)
def test_kernel_temporal_merge_matches_float64_and_oracle(gpu, orc, which, W, H, fc):
    frt = gpu
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    oinp, oout = oracle_temporal(frt, orc, which, W, H, fc)
    r = frt.Renderer(fs, W, H, max_depth=1)
    inp, out = run_temporal(IO(r, H, cam, False), W, H, fc, mats, view_pos, 7000 * W + 13 * H + fc)
    inp["cand"] = r.read_buffer(CANDIDATE, 0).view(f32).reshape(H, W, 4)        # what T-trace handed to T-merge
    worst, amb, merged = check_temporal(inp, out, W, H, fc, view_pos, mats)
    print(f" kernel temporal {which} {W}x{H} f{fc}: worst residual / bound {worst[0]:.3f} (long chains {worst[1]:.3f}); ambiguous {amb:.3%}")
    for k in oinp:
        if k != "cand":
            assert _same(inp[k], oinp[k]), f"temporal input {k} differs from the oracle's"
    surf = inp["gpos"][..., 3] >= 0
    assert _same(inp["cand"][..., 3][surf], oinp["cand"][..., 3][surf]), "the candidate's p_hat differs from the oracle's"
    lit = surf & (inp["cand"][..., 3] > 0)
    assert _same(inp["cand"][..., :3][lit], oinp["cand"][..., :3][lit]), "the candidate's v1 differs from the oracle's"
    assert _same(out, oout), "the stored temporal reservoirs differ from the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("which,W,H,fc", CASES, ids=IDS)
def test_kernel_spatial_reuse_matches_float64_and_oracle(gpu, orc, which, W, H, fc):
    frt = gpu
    fs, _, cam, view_pos, mats = _setup(frt, orc, which, W, H, fc)
    oinp, oout, oraw = oracle_spatial(frt, orc, which, W, H, fc)
    r = frt.Renderer(fs, W, H, max_depth=1)
    inp, out, raw = run_spatial(IO(r, H, cam, False), W, H, fc, mats, view_pos, 9000 * W + 17 * H + fc)
    worst, amb, merges = check_spatial(inp, out, raw, W, H, fc, view_pos, mats, tris_of(fs, which))
    print(f" kernel spatial {which} {W}x{H} f{fc}: worst residual / bound {worst[0]:.3f} (long chains {worst[1]:.3f}); ambiguous {amb:.3%}")
    for k in oinp:
        assert _same(inp[k], oinp[k]), f"spatial input {k} differs from the oracle's"
    assert _same(out, oout), "the spatial reservoirs differ from the oracle's"
    assert _same(raw, oraw), "the radiance target differs from the oracle's"
