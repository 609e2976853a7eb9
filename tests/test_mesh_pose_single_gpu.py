"""The single-mesh posing calls as a batch of one mesh (include/frt.h: frt_renderer_set_mesh_pose, _set_mesh_pose_ex, _set_mesh_morph_weights; DESIGN.md
section 11, "Posing several meshes"): the shapes at which one segment of the batch's launches can go wrong where a launch sized and addressed by one mesh
could not. A 4-vertex quad bound with 256 joints and 300 morph targets — more palette columns (1024) and more weights than vertices, so the tests of a
device palette and of device weights run in threads far beyond the last vertex, in blocks a launch sized by the vertices would not have — a 257-vertex
strip (one vertex past a block of 256) with 2 joints and 2 targets, and a mesh without an instance. Every assertion is against the host scene, never
against another route on the device. Tiny frames."""
import numpy as np
import pytest
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_normals_gpu import check_replica
from test_mesh_skin_gpu import torch_dev, _up, _replica, EVERY      # noqa: F401  (torch_dev: a fixture)
from _mesh_calls import F, QUAD, STRIP, SPARE, pose_scene, strip
from _skin_model import make_skin, make_palette
from _morph_model import make_targets, make_weights

pytestmark = pytest.mark.gpu
W = H = 16
NVERTS = {QUAD: 4, STRIP: 257, SPARE: 6}
BOUND = {QUAD: (256, 300), STRIP: (2, 2), SPARE: (2, 2)}      # mesh -> (joints, targets)
KINDS = ("pose", "morph", "pose and morph")


def _zigzag(frt, n):
    """A strip of n vertices in the plane y = 0 whose vertices alternate between z = -0.25 and z = 0.25: n - 2 triangles, normals +y."""
    xs = np.linspace(-0.5, 0.5, n, dtype=F)
    pos = np.array([[x, 0.0, -0.25 if k % 2 == 0 else 0.25, 1.0] for k, x in enumerate(xs)], F)
    att = np.zeros((n, 8), F)
    att[:, 0:2] = frt.geometry.encode_octahedral_normal([0.0, 1.0, 0.0])
    att[:, 2] = pos[:, 0] + F(0.5); att[:, 3] = pos[:, 2] * F(2.0) + F(0.5)
    att[:, 4:8] = (1.0, 0.0, 0.0, 1.0)
    idx = [(k, k + 1, k + 2) if k % 2 == 0 else (k, k + 2, k + 1) for k in range(n - 2)]
    return frt.geometry.Geometry(pos, att, np.array(idx, np.uint32).reshape(-1))


def _bound(frt):
    """(renderer, host scene): pose_scene over the three meshes, one frame rendered, every mesh bound on both with BOUND's counts. No vertex of the quad
    names its last joint."""
    meshes = [frt.geometry.create_plane(), _zigzag(frt, NVERTS[STRIP]), strip(frt, 3)]
    assert [len(g.positions) for g in meshes] == [NVERTS[m] for m in (QUAD, STRIP, SPARE)]
    fs, _ = pose_scene(frt, meshes=meshes)
    r = frt.Renderer(fs, W, H, max_depth=4)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    for m, (nj, nt) in BOUND.items():
        j, w = make_skin(NVERTS[m], nj, seed=m)
        if m == QUAD:
            j[j == nj - 1] = nj - 2
        for x in (r, fs):
            x.set_mesh_skin(m, j, w, num_joints=nj)
            x.set_mesh_morph_targets(m, make_targets(NVERTS[m], nt, seed=m))
    check_replica(frt, r, fs, "after the bind calls")
    return r, fs


def _inputs(m, kind, phase, bound=None):
    """(palette or None, weights or None) for the counts mesh `m` is bound with. Of two targets the second is all zeros and make_weights gives the first the weight 0: such a morph would
    move nothing, so the first weight is replaced."""
    nj, nt = bound or BOUND[m]
    pal, wts = (make_palette(nj, phase) if kind != "morph" else None), (make_weights(nt, phase) if kind != "pose" else None)
    if wts is not None and nt == 2:
        wts[0] = F(0.375) + F(0.05) * F(phase)
    return pal, wts


def _call(x, m, kind, pal, wts, normals):
    if kind == "morph":
        x.set_mesh_morph_weights(m, wts, normals=normals)
    elif kind == "pose":
        x.set_mesh_pose(m, pal, normals=normals)
    else:
        x.set_mesh_pose(m, pal, normals=normals, morph_weights=wts)


def _pose_both(frt, r, fs, up, m, kind, phase, on_device, normals, what, bound=None):
    """One single-mesh call on the renderer (host arrays, or device tensors through `up`) and on the host scene; then the replica is the host scene's."""
    pal, wts = _inputs(m, kind, phase, bound)
    _call(r, m, kind, up(pal) if on_device and pal is not None else pal, up(wts) if on_device and wts is not None else wts, normals)
    _call(fs, m, kind, pal, wts, normals)
    check_replica(frt, r, fs, what)


def test_every_single_call_equals_the_host_scene(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    r, fs = _bound(frt)
    up = lambda a: _up(torch, dev, a)
    start = r.read_scene("tri_slots").tobytes()
    n = 0
    for normals in ("keep", "recompute"):
        for kind in KINDS:
            for on_device in (False, True):
                for m in (QUAD, STRIP):      # 4 vertices, then 257: the part of the scratch in use shrinks and regrows from call to call
                    n += 1
                    _pose_both(frt, r, fs, up, m, kind, 0.1 * n, on_device, normals, f"{n}: {kind}, {'device' if on_device else 'host'} inputs, {normals}, mesh {m}")
    assert n == 24 and r.deform_rejects() == 0 and r.read_scene("tri_slots").tobytes() != start


def test_the_last_device_weight_and_the_last_palette_column_reject(gpu, torch_dev):
    """The quad's device inputs are tested by threads 299 (the last weight) and 1023 (the last float4 of the palette): the second block and the fourth
    of launches over 4 vertices. The palette's NaN sits in row 3 of the last column of a joint no vertex names: no posed position can show it."""
    frt = gpu
    torch, dev = torch_dev
    r, fs = _bound(frt)
    up = lambda a: _up(torch, dev, a)
    _pose_both(frt, r, fs, up, QUAD, "pose and morph", 0.3, True, "recompute", "a good call first")
    before = _replica(r)
    nj, nt = BOUND[QUAD]
    bad_w = make_weights(nt, 0.5); bad_w[nt - 1] = np.nan
    bad_p = make_palette(nj, 0.5); bad_p[nj - 1, 15] = np.nan
    good_p, good_w = make_palette(nj, 0.6), make_weights(nt, 0.6)
    calls = [("morph", None, bad_w, "keep"), ("pose", bad_p, None, "recompute"), ("pose and morph", good_p, bad_w, "recompute"), ("pose and morph", bad_p, good_w, "keep")]
    for k, (kind, pal, wts, normals) in enumerate(calls):
        _call(r, QUAD, kind, None if pal is None else up(pal), None if wts is None else up(wts), normals)
        assert r.deform_rejects() == k + 1, f"rejected call {k}"
        now = _replica(r)
        for w in EVERY:
            assert now[w] == before[w], f"rejected call {k}: {w} changed"
    check_replica(frt, r, fs, "after the rejected calls")
    _pose_both(frt, r, fs, up, QUAD, "pose and morph", 0.7, True, "keep", "a good call afterwards")
    assert r.deform_rejects() == len(calls)


def test_the_mesh_without_an_instance(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    r, fs = _bound(frt)
    up = lambda a: _up(torch, dev, a)
    slots, attrs = r.read_scene("tri_slots").tobytes(), r.read_scene("attributes").tobytes()
    for k, (kind, on_device) in enumerate((("pose", False), ("pose and morph", True), ("morph", True))):
        _pose_both(frt, r, fs, up, SPARE, kind, 0.4 + k, on_device, "recompute", f"{kind} on the mesh without an instance")
        assert r.read_scene("tri_slots").tobytes() == slots
        assert r.read_scene("attributes").tobytes() != attrs      # (the recomputed normals follow the posed positions: the flat strip is bent)
    assert r.deform_rejects() == 0
    # the posed positions themselves: an instance of the mesh, added afterwards on both sides, has the host scene's triangles
    from frt.scenes import _T, _S, _mul
    m = _mul(_T(-0.3, 0.2, 0.1), _S(0.5))
    assert r.add_instances(SPARE, 0, m) == fs.add_instances(SPARE, 0, m) == 3
    check_replica(frt, r, fs, "an instance of the posed mesh", rebuilt=True)


def test_single_calls_around_a_batch(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    r, fs = _bound(frt)
    up = lambda a: _up(torch, dev, a)
    nj, nt = BOUND[STRIP]
    for x in (r, fs):      # a binding both meshes can be posed under at once
        x.set_mesh_skin(QUAD, *make_skin(NVERTS[QUAD], nj, seed=7), num_joints=nj)
        x.set_mesh_morph_targets(QUAD, make_targets(NVERTS[QUAD], nt, seed=7))
    _pose_both(frt, r, fs, up, STRIP, "pose and morph", 0.2, True, "recompute", "a single call")
    pal, wts = make_palette(nj, 0.5), make_weights(nt, 0.5)
    r.set_mesh_poses([STRIP, QUAD], up(pal), up(wts)); fs.set_mesh_poses([STRIP, QUAD], pal, wts)
    check_replica(frt, r, fs, "the batch over both meshes")
    _pose_both(frt, r, fs, up, QUAD, "pose", 0.8, False, "keep", "a single call on the smaller mesh", bound=(nj, nt))
    _pose_both(frt, r, fs, up, STRIP, "morph", 0.9, True, "recompute", "a single call again")
    assert r.deform_rejects() == 0
