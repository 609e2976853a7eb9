"""Morph targets on the device (include/frt.h: frt_renderer_set_mesh_morph_targets, frt_renderer_set_mesh_morph_weights, frt_renderer_set_mesh_pose_ex;
DESIGN.md section 11, "Morph targets"): after the same bind and the same morphs the replica equals the host scene bit for bit — on the host-built tree
and on a rebuilt one — and the frames equal those of a renderer over a scene built from scratch with the numpy model's positions; weights given as a
device tensor give what the host array gives, in the plain and in the combined call; a non-finite device weight or an overflowing morph is rejected on
the device as data, counted, and leaves the replica alone; morph and skin compose; targets follow remove_meshes; and a MultiRenderer's strips morph
alike. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform, cornell_with, PLANE, CUBE, SPHERE
from test_mesh_deform_gpu import _three_spheres
from test_mesh_skin_gpu import torch_dev, check_replica, _replica, _up, _both, EVERY, W, H      # noqa: F401  (torch_dev: a fixture)
from _skin_model import make_skin, make_palette, scene_with_a_spare_mesh
from _morph_model import F, morph_model, make_targets, make_weights, overflowing_weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["cornell", "three spheres"])
def test_replica_equals_the_host_scene(gpu, torch_dev, which):
    frt = gpu
    torch, dev = torch_dev
    if which == "cornell":      # the sphere (642 vertices: 2.5 blocks, T = 9), the cube (24, T = 1), the plane (4, T = 70: more weights than vertices)
        fs, meshes, ids = frt.scenes.create_cornell_box(), cornell_meshes(frt), ((SPHERE, 9), (CUBE, 1), (PLANE, 70))
        assert [len(meshes[m].positions) for m, _ in ids] == [642, 24, 4]
    else:                       # three instances, one mirrored, of mesh 1 (162 vertices: not a multiple of 64)
        (fs, meshes), ids = _three_spheres(frt), ((1, 3),)
        assert len(meshes[1].positions) == 162 and fs.get("instances")[:, 4].any()
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    start = r.read_scene("tri_slots").tobytes()
    for m, nt in ids:
        _both(r, fs, "set_mesh_morph_targets", m, make_targets(len(meshes[m].positions), nt))
    assert r.read_scene("tri_slots").tobytes() == start      # binding changes no triangle
    for m, nt in ids:           # two morphs back to back, no sync in between: the second reuses the scratch and the staging of the first
        a, b = make_weights(nt, 0.2), make_weights(nt, 0.7)
        r.set_mesh_morph_weights(m, a); r.set_mesh_morph_weights(m, b)
        fs.set_mesh_morph_weights(m, a); fs.set_mesh_morph_weights(m, b)
    check_replica(frt, r, fs, which)      # (reading "normals" makes the pool of decoded normals: the calls below keep it up as well)
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    for m, nt in ids:           # device weights: with T = 70 on the 4-vertex plane the launch is sized by the weights
        w = make_weights(nt, 1.1)
        r.set_mesh_morph_weights(m, _up(torch, dev, w), normals="keep")
        fs.set_mesh_morph_weights(m, w, normals="keep")
    check_replica(frt, r, fs, f"{which}, normals kept, device weights")
    assert r.deform_rejects() == 0
    # a set_mesh_vertices in between leaves the base (a device copy made at the bind call) alone
    m, nt = ids[0]
    d = deform(frt, meshes[m], 0.5)
    _both(r, fs, "set_mesh_vertices", m, d.positions, d.attributes)
    _both(r, fs, "set_mesh_morph_weights", m, make_weights(nt, 1.3))
    check_replica(frt, r, fs, f"{which}, after set_mesh_vertices")
    r.rebuild_tree("sah")
    for m, nt in ids:
        _both(r, fs, "set_mesh_morph_weights", m, make_weights(nt, 1.7))
        _both(r, fs, "set_mesh_morph_weights", m, make_weights(nt, 1.9), normals="keep")
    check_replica(frt, r, fs, f"{which}, after rebuild_tree", rebuilt=True)


def test_frames_equal_a_scene_built_from_scratch(gpu):
    frt = gpu
    base = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
    meshes = list(base)
    for m, nt in ((SPHERE, 9), (CUBE, 1)):
        deltas, w = make_targets(len(base[m].positions), nt), make_weights(nt, 0.4)
        _both(r, fs, "set_mesh_morph_targets", m, deltas)
        _both(r, fs, "set_mesh_morph_weights", m, w)
        mi = fs.get("mesh_infos")[m]
        p = morph_model(base[m].positions, deltas, w)
        meshes[m] = frt.geometry.Geometry(p, fs.get("attributes")[mi[0]:mi[0] + len(p)].copy(), base[m].indices)
    fresh = cornell_with(frt, meshes)
    assert fresh.get("shade_tris").tobytes() == fs.get("shade_tris").tobytes()
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "a morphed mesh vs a build from scratch")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])


@pytest.mark.parametrize("normals", ["recompute", "keep"])
def test_device_tensor_equals_host_array(gpu, torch_dev, normals):
    """The plain morph call and the combined call, each with host arrays on renderer a and device tensors on renderer b."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    base = cornell_meshes(frt)
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    a.render(cam); b.render(cam)
    a.read_scene("normals"); b.read_scene("normals")
    start = _replica(b)
    for m, nt in ((SPHERE, 9), (PLANE, 70), (SPHERE, 9)):      # 642 vertices, 4 (fewer than the weights), and the sphere again with no sync in between
        deltas, w = make_targets(len(base[m].positions), nt), make_weights(nt, 0.6 + m)
        for r in (a, b):
            r.set_mesh_morph_targets(m, deltas)
        a.set_mesh_morph_weights(m, w, normals=normals)
        b.set_mesh_morph_weights(m, _up(torch, dev, w), normals=normals)
    got, want = _replica(b), _replica(a)
    for w in EVERY:
        assert got[w] == want[w], w
    assert got["tri_slots"] != start["tri_slots"] and b.deform_rejects() == 0
    # the combined call: both inputs from the host, both from the device
    skin, pal, w = make_skin(642, 70), make_palette(70, 0.3), make_weights(9, 0.8)
    for r in (a, b):
        r.set_mesh_skin(SPHERE, *skin, num_joints=70)
    a.set_mesh_pose(SPHERE, pal, normals=normals, morph_weights=w)
    b.set_mesh_pose(SPHERE, _up(torch, dev, pal), normals=normals, morph_weights=_up(torch, dev, w))
    mid = got
    got, want = _replica(b), _replica(a)
    for x in EVERY:
        assert got[x] == want[x], f"combined: {x}"
    assert got["tri_slots"] != mid["tri_slots"] and b.deform_rejects() == 0
    with pytest.raises(TypeError, match="both"):
        b.set_mesh_pose(SPHERE, _up(torch, dev, pal), morph_weights=w)
    with pytest.raises(TypeError, match="both"):
        b.set_mesh_pose(SPHERE, pal, morph_weights=_up(torch, dev, w))
    a.clear(); b.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "device weights vs host weights")


def test_bad_morphs_are_rejected_on_the_device(gpu, torch_dev):
    """Ordinary inputs that the device has to turn into a counted rejection: nothing of the call is applied."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    deltas = make_targets(n, 9)
    assert not deltas[8].any()                                      # target 8 moves nothing
    r, ref = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    for x in (r, ref):
        x.set_mesh_morph_targets(SPHERE, deltas)
    r.set_mesh_skin(SPHERE, *make_skin(n, 3), num_joints=3)
    assert r.deform_rejects() == 0
    start = _replica(r)
    good = make_weights(9, 0.8)
    nan_used = good.copy(); nan_used[2] = np.nan                    # a target that moves vertices
    inf_zero = good.copy(); inf_zero[8] = np.inf                    # the all-zero target: 0 * inf is a NaN, and the weight test sees it as well
    ninf_zero = good.copy(); ninf_zero[8] = -np.inf
    calls = [(_up(torch, dev, nan_used), "recompute"), (_up(torch, dev, inf_zero), "keep"), (_up(torch, dev, ninf_zero), "recompute")]
    for k, (w, normals) in enumerate(calls):
        r.set_mesh_morph_weights(SPHERE, w, normals=normals)
        assert r.deform_rejects() == k + 1
        now = _replica(r)
        for x in EVERY:
            assert now[x] == start[x], f"rejected call {k}: {x} changed"
    r.set_mesh_pose(SPHERE, _up(torch, dev, make_palette(3)), morph_weights=_up(torch, dev, inf_zero))      # the combined call rejects it too
    assert r.deform_rejects() == 4 and _replica(r) == start
    for w in (nan_used, inf_zero, ninf_zero):                       # the host form of these: refused, not counted
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_morph_weights(SPHERE, w)
    # finite deltas and weights whose sum overflows: from the host and from the device
    big_d, big_w = overflowing_weights(n, 9)
    assert not np.isfinite(morph_model(cornell_meshes(frt)[SPHERE].positions, big_d, big_w)).all()
    r.set_mesh_morph_targets(SPHERE, big_d)
    for k, w in enumerate((big_w, _up(torch, dev, big_w))):
        r.set_mesh_morph_weights(SPHERE, w, normals=("keep", "recompute")[k])
        assert r.deform_rejects() == 5 + k
        now = _replica(r)
        for x in EVERY:
            assert now[x] == start[x], f"overflowing call {k}: {x} changed"
    # a bad call and a good one back to back, no sync: the good one applies fully, the counter moves by exactly one
    r.set_mesh_morph_targets(SPHERE, deltas)
    r.set_mesh_morph_weights(SPHERE, _up(torch, dev, nan_used))
    r.set_mesh_morph_weights(SPHERE, _up(torch, dev, good))
    ref.read_scene("normals")
    ref.set_mesh_morph_weights(SPHERE, good)
    assert r.deform_rejects() == 7 and ref.deform_rejects() == 0
    got, want = _replica(r), _replica(ref)
    for x in EVERY:
        assert got[x] == want[x], x
    assert got["tri_slots"] != start["tri_slots"]


def test_morph_then_skin_equals_the_host_scene(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    _both(r, fs, "set_mesh_morph_targets", SPHERE, make_targets(n, 9))
    _both(r, fs, "set_mesh_skin", SPHERE, *make_skin(n, 70), num_joints=70)
    start = r.read_scene("tri_slots").tobytes()
    for phase, normals in ((0.2, "recompute"), (0.7, "recompute"), (1.1, "keep")):      # the first two back to back
        r.set_mesh_pose(SPHERE, make_palette(70, phase), normals=normals, morph_weights=make_weights(9, phase))
    for phase, normals in ((0.2, "recompute"), (0.7, "recompute"), (1.1, "keep")):
        fs.set_mesh_pose(SPHERE, make_palette(70, phase), normals=normals, morph_weights=make_weights(9, phase))
    check_replica(frt, r, fs, "morph, then skin")
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    _both(r, fs, "set_mesh_morph_weights", SPHERE, make_weights(9, 1.5))                # the three calls share the scratch buffers: each alone again
    _both(r, fs, "set_mesh_pose", SPHERE, make_palette(70, 1.6))
    _both(r, fs, "set_mesh_pose", SPHERE, make_palette(70, 1.7), morph_weights=make_weights(9, 1.7))
    check_replica(frt, r, fs, "morph, pose, and both")


def test_refusals(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    lib = frt.lib()
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    deltas, w = make_targets(n, 3), make_weights(3)
    t = _up(torch, dev, w)
    r = frt.Renderer(fs, W, H)
    start = _replica(r)
    for x in (w, t):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_morph_weights(SPHERE, x)                     # a mesh with no targets
    nan_d = deltas.copy(); nan_d[0, 0, 0] = np.nan
    for args in ((99, deltas), (SPHERE, deltas[:, :-1]), (SPHERE, nan_d), (SPHERE, deltas[:0])):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_morph_targets(*args)
    assert lib.frt_renderer_set_mesh_morph_targets(r._h, SPHERE, deltas.ctypes.data, n, 4097) == -1
    r.set_mesh_morph_targets(SPHERE, deltas)
    bad = [make_weights(4), _up(torch, dev, make_weights(4)), w[:2], t[:2].contiguous(),      # a wrong target count
           t.double(), t.half(), t.reshape(3, 1), torch.stack([t, t], 1)[:, 0]]                # a wrong dtype, shape or layout
    for x in bad:
        with pytest.raises(frt.FrtError):
            r.set_mesh_morph_weights(SPHERE, x)
    for x in (w, t):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_morph_weights(99, x)
        with pytest.raises(frt.FrtError, match="normals must be"):
            r.set_mesh_morph_weights(SPHERE, x, normals="smooth")
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_pose(SPHERE, make_palette(3) if x is w else _up(torch, dev, make_palette(3)), morph_weights=x)      # no skin
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, w.ctypes.data, 3, frt.DEFORM_DEVICE) == -1        # host memory is not device memory
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, t.data_ptr() + 2, 3, frt.DEFORM_DEVICE) == -1    # not 4-byte aligned
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, None, 3, frt.DEFORM_DEVICE) == -1
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, None, 3, 0) == -1
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, w.ctypes.data, 3, 4) == -1                        # an unknown flag bit
    # inside an open frame
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, w.ctypes.data, 3, 0) == -4
    assert lib.frt_renderer_set_mesh_morph_weights(r._h, SPHERE, t.data_ptr(), 3, frt.DEFORM_DEVICE) == -4
    assert lib.frt_renderer_set_mesh_morph_targets(r._h, SPHERE, deltas.ctypes.data, n, 3) == -4
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert r.deform_rejects() == 0
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], x
    r.set_mesh_morph_targets(SPHERE, None)                          # the targets leave
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_morph_weights(SPHERE, w)


def test_targets_follow_remove_meshes(gpu):
    """Meshes 1 (unused), 2 and 3 get targets, mesh 1 is removed: 2 and 3 become 1 and 2 and must morph with their own deltas and bases — a stale list
    would morph the 162-vertex sphere with the crystal's buffer."""
    frt = gpu
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    t1, t2, t3 = make_targets(len(meshes[1].positions), 3), make_targets(len(meshes[2].positions), 70), make_targets(len(meshes[3].positions), 3, seed=1)
    for m, t in ((1, t1), (2, t2), (3, t3)):
        _both(r, fs, "set_mesh_morph_targets", m, t)
    _both(r, fs, "set_mesh_morph_weights", 2, make_weights(70, 0.1))
    _both(r, fs, "remove_meshes", 1)
    w70, w3 = make_weights(70, 0.3), make_weights(3, 0.6)
    _both(r, fs, "set_mesh_morph_weights", 1, w70)
    _both(r, fs, "set_mesh_morph_weights", 2, w3)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_morph_weights(1, w3)                             # (the crystal's three targets left with it)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_morph_weights(0, w3)
    assert r.pool_counts()["meshes"] == 3
    for w in ("indices", "mesh_infos"):
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w
    check_replica(frt, r, fs, "after remove_meshes", rebuilt=True)      # (the host scene built its tree again: the slots are compared by triangle id)


def test_multi_renderer(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    deltas, w = make_targets(n, 9), make_weights(9, 0.2)
    skin, pal = make_skin(n, 3), make_palette(3, 0.2)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        x.set_mesh_morph_targets(SPHERE, deltas)
        x.set_mesh_morph_weights(SPHERE, w)
        x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    for x in (multi, one):
        x.set_mesh_skin(SPHERE, *skin, num_joints=3)
        x.set_mesh_pose(SPHERE, pal, morph_weights=make_weights(9, 0.5))
        x.clear()
        x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    t, tp = _up(torch, dev, w), _up(torch, dev, pal)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_morph_weights(SPHERE, t)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_pose(SPHERE, pal, morph_weights=t)
    lib = frt.lib()
    assert lib.frt_multi_renderer_set_mesh_morph_weights(multi._h, SPHERE, t.data_ptr(), 9, frt.DEFORM_DEVICE) == -1      # the device flag on strips
    assert lib.frt_multi_renderer_set_mesh_pose_ex(multi._h, SPHERE, tp.data_ptr(), 3, t.data_ptr(), 9, frt.DEFORM_DEVICE) == -1
    assert lib.frt_multi_renderer_set_mesh_morph_weights(multi._h, SPHERE, w.ctypes.data, 8, 0) == -1
    assert lib.frt_multi_renderer_set_mesh_morph_targets(multi._h, SPHERE, deltas.ctypes.data, n - 1, 9) == -1
