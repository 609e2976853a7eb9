"""The G-buffer pass (gbuffer.wgsl main) against its float64 restatement (tests/_wgsl_f64.py), pixel by pixel, on three implementations:
the oracle and the host-compiled product (CPU suite) and libfrt.so (-m gpu). Unlike the parity tests, nothing on the reference side was
written from the product's or the oracle's reading of the shader, so a misreading shared by both is caught here.
Scenes: (a) the Cornell Box (rotated, non-uniformly scaled box; checker texture); (b) non-uniform scale + rotation, shear, a mirrored
instance and a plane seen from behind; (c) colour / occlusion / normal layers with uv outside [0, 1] and vertex normals on the
octahedral fold. Cameras: static, moved and turned (motion != 0), looking straight down the -y axis."""
import ctypes as C
import numpy as np
import pytest
import _wgsl_f64 as R

SIZES = [(1, 1), (3, 2), (7, 5), (16, 16), (17, 33), (128, 72)]
# tolerances (measured worst residuals over every case of the CPU suite are printed by each test and listed in the pull request)
POS_ULP = 16            # |pos - pos64| / max(1, |pos64|, t) * |cos(incidence)|, in units of 2^-23: an f32 ray's direction error moves
                        # the hit along the surface by t / |cos| times itself (|cos| floored at 0.05: at most 20x the bound)
NORMAL_ABS = 4e-5       # encoded normal, plus how much it moves when uv moves by UV_ABS (normal-mapped pixels)
UV_ABS = 2e-5
MOTION_ABS, MOTION_REL = 1e-5, 1e-5
ALBEDO_EDGE = 1e-4      # unorm8 albedo: the rounding of [a - e, a + e], e = this + how much a moves when uv moves by UV_ABS
ON_EDGE_MAX = 0.015     # rays through an edge to within f32 rounding (whole pixel diagonals of the Cornell Box seen along its axis)
AMBIGUOUS_MAX = 0.01    # share of pixels float64 cannot decide robustly (edges, near-equal t), over all sizes of a case; rays that meet an
                        # edge to within f32 rounding are counted apart (the Cornell Box seen from its axis puts whole pixel diagonals on its corner lines)


# ------------------------------------------------------------------------------------------------ scenes (every call to both libraries)
def _tri_mesh(pos3, nrm_enc, uv, tangent, idx):
    n = len(pos3)
    p = np.zeros((n, 4), np.float32); p[:, :3] = pos3; p[:, 3] = 1.0
    a = np.zeros((n, 8), np.float32); a[:, 0:2] = nrm_enc; a[:, 2:4] = uv; a[:, 4:8] = tangent
    return p, a, np.asarray(idx, np.uint32)


def _m4(A, t=(0, 0, 0)):
    """3x3 linear part + translation -> column-major 16 floats (what add_instance takes)."""
    M = np.eye(4); M[:3, :3] = A; M[:3, 3] = t
    return np.asarray(M.T, np.float32).reshape(16)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    Rm = np.eye(3); Rm[i, i] = Rm[j, j] = c; Rm[i, j] = -s; Rm[j, i] = s
    return Rm


class _Textures:
    def __init__(self):
        self.layers = R.default_textures()

    def add(self, b, kind, img):
        img = np.ascontiguousarray(img, np.uint8)
        a = (b.fb.add_color_texture if kind == 0 else b.fb.add_data_texture)(img)
        o = b.orc.L.orc_scene_add_texture(b.oh, kind, img.ctypes.data)
        assert a == o == len(self.layers["color" if kind == 0 else "data"])
        self.layers["color" if kind == 0 else "data"].append(img)
        return a


def _light(frt, b):
    import _scenes
    b.add_light(_scenes._quad_light(frt, (0, 0.99, 0), 0.25, (1, 1, 1, 10)))


def scene_cornell(frt, orc):
    fs, os_ = frt.scenes.create_cornell_box(), orc.cornell()
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    return fs, os_, R.default_textures()


def scene_transforms(frt, orc):
    import _scenes
    b = _scenes.DualBuilder(frt, orc)
    plane = b.add_mesh(*_scenes._geo(frt, "create_plane"))
    sphere = b.add_mesh(*_scenes._geo(frt, "create_sphere", 2))
    cube = b.add_mesh(*_scenes._geo(frt, "create_cube"))
    crystal = b.add_mesh(*_scenes._geo(frt, "create_crystal"))
    mats = [b.add_material(frt.material_new(c)) for c in ([0.8, 0.3, 0.2, 1], [0.2, 0.7, 0.3, 1], [0.3, 0.4, 0.9, 1], [0.9, 0.9, 0.2, 1], [0.5, 0.5, 0.5, 1])]
    b.add_instance(sphere, mats[0], _m4(_rot(2, 0.7) @ _rot(0, 0.4) @ np.diag([1.0, 0.3, 2.0]) * 0.5, (-0.45, 0.25, -0.6)))
    shear = np.array([[1.0, 0.6, 0.0], [0.0, 1.0, 0.0], [0.3, 0.0, 1.0]])
    b.add_instance(cube, mats[1], _m4(_rot(1, 0.5) @ shear * 0.35, (0.5, 0.2, -0.4)))
    mirror = _rot(1, 0.9) @ np.diag([-0.5, 0.45, 0.4])                   # negative determinant
    b.add_instance(crystal, mats[2], _m4(mirror, (0.05, -0.45, -0.2)))
    b.add_instance(sphere, mats[3], _m4(_rot(0, -0.3) @ np.diag([0.3, 0.3, -0.3]), (0.55, -0.5, 0.1)))
    b.add_instance(plane, mats[4], _m4(_rot(0, -1.2) * 1.6, (0.0, -0.2, -1.2)))   # its front face (+y) turned away from the camera
    b.add_instance(plane, mats[4], _m4(np.diag([4.0, 1.0, 4.0]), (0.0, -1.0, 0.0)))
    _light(frt, b)
    fs, os_ = b.build()
    return fs, os_, R.default_textures()


def scene_textured(frt, orc):
    import _scenes
    rng = np.random.default_rng(7)
    b = _scenes.DualBuilder(frt, orc)
    tx = _Textures()
    col = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
    occ = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
    nm = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8); nm[..., 2] = rng.integers(150, 256, (1024, 1024))   # normals mostly up
    c_id, o_id, n_id = tx.add(b, 0, col), tx.add(b, 1, occ), tx.add(b, 1, nm)
    # a quad with uv in [-1.3, 2.7] x [-0.6, 1.9] (Repeat), tangent sign +1 on one triangle and -1 on the other
    P = np.array([[-1, 0, 1], [1, 0, 1], [-1, 0, -1], [1, 0, -1], [-1, 0, 1], [1, 0, -1]], np.float64)
    up = R.encode_octahedral(np.array([[0.0, 1.0, 0.0]]))[0]
    uv = np.array([[-1.3, 1.9], [2.7, 1.9], [-1.3, -0.6], [2.7, -0.6], [-1.3, 1.9], [2.7, -0.6]])
    tg = np.array([[1, 0, 0, 1]] * 3 + [[1, 0, 0, -1]] * 3, np.float64)
    quad = b.add_mesh(*_tri_mesh(P, [up] * 6, uv, tg, [0, 1, 2, 4, 5, 3]))
    m = frt.material_new([0.9, 0.8, 0.7, 1.0]); m.tex_info_0 = c_id | (n_id << 16); m.tex_info_1 = o_id | 0xFFFF0000
    textured = b.add_material(m)
    b.add_instance(quad, textured, _m4(_rot(0, 0.9) @ np.diag([0.8, 1.0, 0.6]), (0.0, 0.0, -0.5)))
    # triangles facing the camera whose vertex normals lie on the octahedral fold: z < 0 with x == 0 (encoded (0.5, -1)) or y == 0
    # (encoded (-1, 0.25)); both decode exactly in f32, and an axis-aligned instance keeps the zero component exactly zero
    F = np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.0, 0.2, 0], [0.3, -0.2, 0], [0.7, -0.2, 0], [0.5, 0.2, 0]], np.float64)
    enc = [[0.5, -1.0]] * 3 + [[-1.0, 0.25]] * 3
    fold = b.add_mesh(*_tri_mesh(F, enc, np.zeros((6, 2)), [[1, 0, 0, 1]] * 6, [0, 1, 2, 3, 4, 5]))
    m2 = frt.material_new([0.6, 0.6, 0.6, 1.0]); m2.tex_info_0 = c_id | 0xFFFF0000
    plain = b.add_material(m2)
    b.add_instance(fold, plain, _m4(np.diag([1.5, 1.2, 1.0]), (-0.4, 0.35, 0.2)))
    _light(frt, b)
    fs, os_ = b.build()
    return fs, os_, tx.layers


SCENES = {"cornell": scene_cornell, "transforms": scene_transforms, "textured": scene_textured}


# ------------------------------------------------------------------------------------------------ cameras
def _uniform(frt, eye, fwd, up, aspect, prev_vp=None):
    """A CameraUniform looking from `eye` along `fwd` (camera.rs:207-256 conventions: right-handed view, 45 degree fovy, z in [0, 1])."""
    eye, fwd = np.asarray(eye, np.float64), np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    s = np.cross(fwd, up); s /= np.linalg.norm(s)
    u = np.cross(s, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -fwd
    view[0, 3], view[1, 3], view[2, 3] = -eye @ s, -eye @ u, eye @ fwd
    h = 1.0 / np.tan(np.radians(45.0) / 2); r = 100.0 / (0.1 - 100.0)
    proj = np.zeros((4, 4)); proj[0, 0] = h / aspect; proj[1, 1] = h; proj[2, 2] = r; proj[2, 3] = r * 0.1; proj[3, 2] = -1.0
    vp = proj @ view
    cu = frt.CameraUniform()
    col = lambda m: np.asarray(m, np.float32).T.reshape(16)
    cu.view_proj[:] = col(vp); cu.view_inverse[:] = col(np.linalg.inv(view)); cu.proj_inverse[:] = col(np.linalg.inv(proj))
    cu.prev_view_proj[:] = col(vp if prev_vp is None else prev_vp)
    cu.view_pos[:] = [eye[0], eye[1], eye[2], 1.0]
    cu.frame_count, cu.num_lights = 0, 1
    return cu, vp


def camera(frt, which, aspect):
    if which == "static":
        cu = frt.CameraController().build_uniform(aspect, 0, 1)
        cu.num_lights = 1
        return cu
    if which == "moving":          # previous frame: further back, lower and turned; this frame moved and turned
        _, prev = _uniform(frt, (0.15, -0.1, 3.3), (-0.12, 0.05, -1.0), (0, 1, 0), aspect)
        return _uniform(frt, (-0.1, 0.12, 2.8), (0.08, -0.06, -1.0), (0, 1, 0), aspect, prev)[0]
    if which == "down":            # straight down the -y axis
        return _uniform(frt, (0.0, 2.4, -0.3), (0.0, -1.0, 0.0), (0, 0, -1), aspect)[0]
    raise ValueError(which)


CAMERAS = ["static", "moving", "down"]

_REF = {}


def reference(frt, scene_name, cam_name, W, H, sc, textures, mis=()):
    """gbuffer_f64 for one case, cached per process (the same reference serves every target)."""
    key = (scene_name, cam_name, W, H, tuple(sorted(mis)))
    if key not in _REF:
        _REF[key] = R.gbuffer_f64(sc, camera(frt, cam_name, W / H), W, H, textures, mis)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ comparison
def residuals(got, ref):
    """got: dict gpos (H, W, 4) f32, gnormal (H, W, 4) f32, galbedo (H, W, 4) u8, gmotion (H, W, 2) f32. Returns the per-quantity worst
    residuals on decidable pixels and a list of violations (empty: the implementation agrees with the float64 reference)."""
    ok = ~ref["ambiguous"]
    bad = []
    miss = got["gpos"][..., 3] == -1.0
    if (miss[ok] != ref["miss"][ok]).any():
        bad.append(f"miss mask differs at {int((miss != ref['miss'])[ok].sum())} pixels")
    mat = np.where(miss, -1.0, got["gpos"][..., 3])
    if (mat[ok] != ref["mat_id"][ok]).any():
        bad.append(f"mat_id differs at {int((mat != ref['mat_id'])[ok].sum())} pixels")
    h = ok & ~ref["miss"] & ~miss
    r = {"pos_ulp": 0.0, "normal": 0.0, "uv": 0.0, "motion": 0.0, "albedo_off": 0}
    if not h.any():
        return r, bad
    scale = np.maximum(np.maximum(1.0, np.abs(ref["pos"]).max(-1)), ref["t"]) / np.maximum(ref["cos"], 0.05)
    pos = np.abs(got["gpos"][..., :3] - ref["pos"]).max(-1) / scale / 2.0 ** -23
    nrm = np.abs(got["gnormal"][..., :2] - ref["enc_normal"]).max(-1)
    nrm_bad = (np.abs(got["gnormal"][..., :2] - ref["enc_normal"]) > NORMAL_ABS + ref["normal_sens"]).any(-1)
    uv = np.abs(got["gnormal"][..., 2:4] - ref["uv"]).max(-1)
    mot = (np.abs(got["gmotion"] - ref["motion"]) / (MOTION_ABS + MOTION_REL * np.abs(ref["motion"]))).max(-1)
    r["pos_ulp"], r["normal"], r["uv"] = float(pos[h].max()), float(nrm[h].max()), float(uv[h].max())
    r["motion"] = float(np.abs(got["gmotion"] - ref["motion"]).max(-1)[h].max())
    a = np.clip(ref["albedo"], 0.0, 1.0) * 255.0
    q = got["galbedo"][..., :3].astype(np.int64)
    want = np.floor(a + 0.5)
    e = (ALBEDO_EDGE + ref["albedo_sens"]) * 255.0
    lo, hi = np.floor(np.clip(a - e, 0, 255) + 0.5), np.floor(np.clip(a + e, 0, 255) + 0.5)
    r["albedo_off"] = int(((q != want).any(-1) & h).sum())
    for name, viol in (("pos", pos > POS_ULP), ("normal", nrm_bad), ("uv", uv > UV_ABS), ("motion", mot > 1.0),
                       ("albedo", ((q < lo) | (q > hi)).any(-1))):
        v = viol & h
        if v.any():
            y, x = np.argwhere(v)[0]
            bad.append(f"{name}: {int(v.sum())} pixels out of tolerance, first at (y={y}, x={x})")
    return r, bad


def _read_oracle(ro):
    return {"gpos": ro.read(0, 0).view(np.float32), "gnormal": ro.read(1, 0).view(np.float32), "galbedo": ro.read(2, 0),
            "gmotion": ro.read(3, 0).view(np.float32)}


def _cases():
    return [(s, c) for s in SCENES for c in CAMERAS]


def run_case(frt, orc, scene_name, cam_name, render_and_read):
    """render_and_read(fs, os_, cam, W, H) -> buffers of frame 0. Asserts every size of the case, prints the worst residuals."""
    fs, os_, tex = SCENES[scene_name](frt, orc)
    sc = R.scene_arrays(fs)
    worst = {"pos_ulp": 0.0, "normal": 0.0, "uv": 0.0, "motion": 0.0, "albedo_off": 0}
    amb = exact = npix = 0
    failures = []
    for W, H in SIZES:
        ref = reference(frt, scene_name, cam_name, W, H, sc, tex)
        got = render_and_read(fs, os_, camera(frt, cam_name, W / H), W, H)
        r, bad = residuals(got, ref)
        failures += [f"{W}x{H}: {b}" for b in bad]
        for k in worst:
            worst[k] = max(worst[k], r[k])
        amb += int((ref["ambiguous"] & ~ref["on_edge"]).sum()); exact += int(ref["on_edge"].sum()); npix += W * H
    print(f"\n{scene_name}/{cam_name}: ambiguous {amb} (+ {exact} on an edge) of {npix} pixels; worst pos {worst['pos_ulp']:.1f} ulp, normal {worst['normal']:.2e}, "
          f"uv {worst['uv']:.2e}, motion {worst['motion']:.2e}, albedo +-1 at {worst['albedo_off']} pixels")
    assert not failures, "; ".join(failures[:8])
    assert amb <= AMBIGUOUS_MAX * npix
    assert exact <= ON_EDGE_MAX * npix
    return worst


def test_reference_scenes_are_what_they_claim(frt, orc):
    """Scene (b) holds a mirrored instance and a shear, scene (c) fold normals; the moving camera has motion, and the cases see them."""
    fs, _, _ = scene_transforms(frt, orc)
    inst = fs.get("instances")
    dets = [np.linalg.det(inst[i, 5:21].view(np.float32).reshape(4, 4)[:3, :3].astype(np.float64)) for i in range(len(inst))]
    assert min(dets) < 0 < max(dets)
    fs, _, tex = scene_textured(frt, orc)
    ref = R.gbuffer_f64(R.scene_arrays(fs), camera(frt, "static", 128 / 72), 128, 72, tex)
    hit = ~ref["miss"]
    assert ((ref["uv"] < 0) | (ref["uv"] > 1)).any(-1)[hit].sum() > 100                       # Repeat addressing reached
    n = ref["normal"]
    on_fold = hit & (n[..., 2] < 0) & ((n[..., 0] == 0) | (n[..., 1] == 0))
    assert on_fold.sum() > 20                                                                   # x or y exactly 0 with z < 0
    mv = R.gbuffer_f64(R.scene_arrays(fs), camera(frt, "moving", 128 / 72), 128, 72, tex)["motion"]
    assert (np.abs(mv[..., 0]) > 1e-3).any() and (np.abs(mv[..., 1]) > 1e-3).any()


@pytest.mark.parametrize("scene_name,cam_name", _cases())
def test_oracle_gbuffer_matches_float64(frt, orc, scene_name, cam_name):
    def go(fs, os_, cam, W, H):
        ro = os_.renderer(W, H, 1, True, 8)
        ro.render_phases(cam, 1, 0, H)
        return _read_oracle(ro)
    run_case(frt, orc, scene_name, cam_name, go)


@pytest.mark.parametrize("scene_name,cam_name", _cases())
def test_hostcheck_gbuffer_matches_float64(frt, orc, hostcheck, scene_name, cam_name):
    def go(fs, os_, cam, W, H):          # the host build has no phase control: a whole frame, then its G-buffer (slot 0 at frame 0)
        rh = hostcheck.renderer(fs, W, H, 1, 8)
        rh.render(cam)
        return {"gpos": rh.read(0, 0).view(np.float32), "gnormal": rh.read(1, 0).view(np.float32), "galbedo": rh.read(2, 0),
                "gmotion": rh.read(3, 0).view(np.float32)}
    run_case(frt, orc, scene_name, cam_name, go)


@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,cam_name", _cases())
def test_kernels_gbuffer_matches_float64(gpu, orc, scene_name, cam_name):
    frt = gpu

    def go(fs, os_, cam, W, H):
        r = frt.Renderer(fs, W, H, max_depth=1)
        r.render_phases(cam, frt.PHASE_GBUFFER)
        got = {"gpos": r.read_buffer(0, 0).view(np.float32), "gnormal": r.read_buffer(1, 0).view(np.float32), "galbedo": r.read_buffer(2, 0),
               "gmotion": r.read_buffer(3, 0).view(np.float32)}
        ro = os_.renderer(W, H, 1, True, 8)          # and bit for bit the oracle's
        ro.render_phases(cam, 1, 0, H)
        want = _read_oracle(ro)
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), f"{W}x{H} {k}: kernel differs from the oracle"
        return got
    run_case(frt, orc, scene_name, cam_name, go)
