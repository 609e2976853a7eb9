"""Skinning on the device (include/frt.h: frt_renderer_set_mesh_skin, frt_renderer_set_mesh_pose; DESIGN.md section 11, "Skinning"): after the same
bind and the same poses the replica equals the host scene bit for bit — on the host-built tree and on a rebuilt one — and the frames equal those of a
renderer over a scene built from scratch with the numpy model's positions; a palette given as a device tensor gives what the host array gives; a
non-finite palette entry or an overflowing pose is rejected on the device as data, counted, and leaves the replica alone; what cannot be a pose is
refused on the host; skins follow remove_meshes; and a MultiRenderer's strips pose alike. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform, cornell_with, PLANE, CUBE, SPHERE
from test_mesh_deform_gpu import _three_spheres
from test_mesh_normals_gpu import check_replica, REPLICA, W, H
from _skin_model import F, skin_model, make_skin, make_palette, overflowing_palette, scene_with_a_spare_mesh

pytestmark = pytest.mark.gpu
EVERY = REPLICA + ("normals",)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda", 0)


def _replica(r):
    return {w: r.read_scene(w).tobytes() for w in EVERY}


def _up(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(dev)


def _both(r, fs, call, *args, **kw):
    getattr(r, call)(*args, **kw); getattr(fs, call)(*args, **kw)


@pytest.mark.parametrize("which", ["cornell", "three spheres"])
def test_replica_equals_the_host_scene(gpu, which):
    frt = gpu
    if which == "cornell":      # the sphere (642 vertices: 2.5 blocks), the plane (4: less than a wave), the cube (24); palettes of 70, 1 and 3 joints
        fs, meshes, ids = frt.scenes.create_cornell_box(), cornell_meshes(frt), ((SPHERE, 70), (PLANE, 1), (CUBE, 3))
        assert [len(meshes[m].positions) for m, _ in ids] == [642, 4, 24]
    else:                       # three instances, one mirrored, of mesh 1 (162 vertices: not a multiple of 64)
        (fs, meshes), ids = _three_spheres(frt), ((1, 3), (0, 1))
        assert len(meshes[1].positions) % 64 and fs.get("instances")[:, 4].any()
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    start = r.read_scene("tri_slots").tobytes()
    for m, nj in ids:
        _both(r, fs, "set_mesh_skin", m, *make_skin(len(meshes[m].positions), nj), num_joints=nj)
    assert r.read_scene("tri_slots").tobytes() == start      # binding changes no triangle
    for m, nj in ids:           # two poses back to back, no sync in between: the second reuses the scratch and the staging of the first
        a, b = make_palette(nj, 0.2), make_palette(nj, 0.7)
        r.set_mesh_pose(m, a); r.set_mesh_pose(m, b.reshape(nj, 4, 4))
        fs.set_mesh_pose(m, a); fs.set_mesh_pose(m, b)
    check_replica(frt, r, fs, which)      # (reading "normals" makes the pool of decoded normals: the calls below keep it up as well)
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    for m, nj in ids:
        _both(r, fs, "set_mesh_pose", m, make_palette(nj, 1.1), normals="keep")
    check_replica(frt, r, fs, f"{which}, normals kept")
    # a set_mesh_vertices in between leaves the bind pose (a device copy made at the bind call) alone
    m, nj = ids[0]
    d = deform(frt, meshes[m], 0.5)
    _both(r, fs, "set_mesh_vertices", m, d.positions, d.attributes)
    _both(r, fs, "set_mesh_pose", m, make_palette(nj, 1.3))
    check_replica(frt, r, fs, f"{which}, after set_mesh_vertices")
    r.rebuild_tree("sah")
    for m, nj in ids:
        _both(r, fs, "set_mesh_pose", m, make_palette(nj, 1.7))
    check_replica(frt, r, fs, f"{which}, after rebuild_tree", rebuilt=True)


def test_frames_equal_a_scene_built_from_scratch(gpu):
    frt = gpu
    base = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
    meshes = list(base)
    for m, nj in ((SPHERE, 70), (CUBE, 3)):
        skin, pal = make_skin(len(base[m].positions), nj), make_palette(nj, 0.4)
        _both(r, fs, "set_mesh_skin", m, *skin, num_joints=nj)
        _both(r, fs, "set_mesh_pose", m, pal)
        mi = fs.get("mesh_infos")[m]
        p = skin_model(base[m].positions, *skin, pal)
        meshes[m] = frt.geometry.Geometry(p, fs.get("attributes")[mi[0]:mi[0] + len(p)].copy(), base[m].indices)
    fresh = cornell_with(frt, meshes)
    assert fresh.get("shade_tris").tobytes() == fs.get("shade_tris").tobytes()
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "a posed mesh vs a build from scratch")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])


@pytest.mark.parametrize("normals", ["recompute", "keep"])
def test_device_tensor_equals_host_array(gpu, torch_dev, normals):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    base = cornell_meshes(frt)
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    a.render(cam); b.render(cam)
    a.read_scene("normals"); b.read_scene("normals")
    start = _replica(b)
    for m, nj in ((SPHERE, 70), (PLANE, 1), (SPHERE, 70)):      # 642 vertices, 4, and the sphere again with no sync in between
        skin, pal = make_skin(len(base[m].positions), nj), make_palette(nj, 0.6 + m)
        for r in (a, b):
            r.set_mesh_skin(m, *skin, num_joints=nj)
        a.set_mesh_pose(m, pal, normals=normals)
        b.set_mesh_pose(m, _up(torch, dev, pal) if m == SPHERE else _up(torch, dev, pal).reshape(nj, 4, 4), normals=normals)
    got, want = _replica(b), _replica(a)
    for w in EVERY:
        assert got[w] == want[w], w
    assert got["tri_slots"] != start["tri_slots"] and b.deform_rejects() == 0
    a.clear(); b.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "a device palette vs a host palette")


def test_palette_from_another_stream(gpu, torch_dev):
    """The palette is the result of kernels enqueued on a side stream just before the call, behind enough other work there that a call which did not
    wait for that stream would read the buffer before it is written (it holds zeros until then)."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    skin, pal = make_skin(n, 70), make_palette(70, 1.1)
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    for r in (a, b):
        r.set_mesh_skin(SPHERE, *skin)
    a.set_mesh_pose(SPHERE, pal)
    src = _up(torch, dev, pal)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        busy = torch.ones((4096, 4096), device=dev)
        for _ in range(100):
            busy = busy * 1.0001 + 0.001
        mats = torch.zeros_like(src)
        mats += src * (busy[0, 0] * 0 + 1)                 # (depends on the work above; the same bits as `src`)
        b.set_mesh_pose(SPHERE, mats)
    got, want = _replica(b), _replica(a)
    for w in EVERY:
        assert got[w] == want[w], w
    assert b.deform_rejects() == 0


def test_bad_poses_are_rejected_on_the_device(gpu, torch_dev):
    """Ordinary inputs that the device has to turn into a counted rejection: nothing of the call is applied."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    joints, weights = make_skin(n, 70)
    joints[joints == 33] = 34                                      # no vertex names joint 33
    assert joints.max() == 69 and (joints == 5).any()
    r, ref = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    for x in (r, ref):
        x.set_mesh_skin(SPHERE, joints, weights, num_joints=70)
    assert r.deform_rejects() == 0
    start = _replica(r)
    good = make_palette(70, 0.8)
    nan_named = good.copy(); nan_named[5, 9] = np.nan              # a joint that vertices name
    inf_unnamed = good.copy(); inf_unnamed[33, 12] = np.inf        # a joint no vertex names: the host form refuses it, the device form rejects it
    inf_row3 = good.copy(); inf_row3[69, 15] = -np.inf             # the last float of the palette, in the row the arithmetic ignores
    over = overflowing_palette(70)
    calls = [(_up(torch, dev, nan_named), "recompute"), (_up(torch, dev, inf_unnamed), "keep"), (_up(torch, dev, inf_row3), "recompute"),
             (_up(torch, dev, over), "recompute"), (over, "keep")]  # finite matrices that overflow: as a device tensor and as a host array
    for k, (m, normals) in enumerate(calls):
        r.set_mesh_pose(SPHERE, m, normals=normals)
        assert r.deform_rejects() == k + 1
        now = _replica(r)
        for w in EVERY:
            assert now[w] == start[w], f"rejected call {k}: {w} changed"
    for m in (nan_named, inf_unnamed, inf_row3):                    # the host form of the first three: refused, not counted
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_pose(SPHERE, m)
    # a bad call and a good one back to back, no sync: the good one applies fully, the counter moves by exactly one
    r.set_mesh_pose(SPHERE, _up(torch, dev, nan_named))
    r.set_mesh_pose(SPHERE, _up(torch, dev, good))
    ref.read_scene("normals")
    ref.set_mesh_pose(SPHERE, good)
    assert r.deform_rejects() == len(calls) + 1 and ref.deform_rejects() == 0
    got, want = _replica(r), _replica(ref)
    for w in EVERY:
        assert got[w] == want[w], w
    assert got["tri_slots"] != start["tri_slots"]


def test_refusals(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    lib = frt.lib()
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    joints, weights = make_skin(n, 3)
    pal = make_palette(3)
    t = _up(torch, dev, pal)
    r = frt.Renderer(fs, W, H)
    start = _replica(r)
    for m in (pal, t):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_pose(SPHERE, m)                              # a mesh without a skin
    big = joints.copy(); big[7, 3] = 3
    neg = weights.copy(); neg[9, 0] = -1.0
    for args in ((99, joints, weights), (SPHERE, joints[:-1], weights[:-1]), (SPHERE, big, weights), (SPHERE, joints, neg)):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_skin(*args, num_joints=3)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_skin(SPHERE, joints, weights, num_joints=0)
    r.set_mesh_skin(SPHERE, joints, weights, num_joints=3)
    bad = [make_palette(4), _up(torch, dev, make_palette(4)), pal[:2], t[:2].contiguous(),       # a wrong joint count
           t.double(), t.half(), t[:, :12].contiguous(), t.t().contiguous().t(), t.reshape(-1)]  # a wrong dtype, shape or layout
    for m in bad:
        with pytest.raises(frt.FrtError):
            r.set_mesh_pose(SPHERE, m)
    for m in (pal, t):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_pose(99, m)
        with pytest.raises(frt.FrtError, match="normals must be"):
            r.set_mesh_pose(SPHERE, m, normals="smooth")
    # (a tensor on another device needs a second device: on a one-GPU machine neither the Python check nor the library's `device != renderer's` check runs here)
    if torch.cuda.device_count() > 1:
        with pytest.raises(frt.FrtError, match="renderer on device 0"):
            r.set_mesh_pose(SPHERE, t.to(torch.device("cuda", 1)))
    # one host and one device argument: each with the other's flag
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, pal.ctypes.data, 3, frt.DEFORM_DEVICE) == -1        # host memory is not device memory
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, t.data_ptr() + 4, 3, frt.DEFORM_DEVICE) == -1       # not 16-byte aligned
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, None, 3, frt.DEFORM_DEVICE) == -1
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, None, 3, 0) == -1
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, pal.ctypes.data, 3, 4) == -1                        # an unknown flag bit
    # inside an open frame
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, pal.ctypes.data, 3, 0) == -4
    assert lib.frt_renderer_set_mesh_pose(r._h, SPHERE, t.data_ptr(), 3, frt.DEFORM_DEVICE) == -4
    assert lib.frt_renderer_set_mesh_skin(r._h, SPHERE, joints.ctypes.data, weights.ctypes.data, n, 3) == -4
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert r.deform_rejects() == 0
    now = _replica(r)
    for w in EVERY:
        assert now[w] == start[w], w
    r.set_mesh_skin(SPHERE, None)                                   # the skin leaves
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_pose(SPHERE, pal)


def test_skins_follow_remove_meshes(gpu):
    """Meshes 1 (unused), 2 and 3 are skinned, mesh 1 is removed: 2 and 3 become 1 and 2 and must pose with their own joints, weights and bind poses —
    a stale list would skin the 162-vertex sphere with the crystal's buffers."""
    frt = gpu
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    s1, s2, s3 = make_skin(len(meshes[1].positions), 3), make_skin(len(meshes[2].positions), 70), make_skin(len(meshes[3].positions), 3, seed=1)
    for m, s in ((1, s1), (2, s2), (3, s3)):
        _both(r, fs, "set_mesh_skin", m, *s)
    _both(r, fs, "set_mesh_pose", 2, make_palette(70, 0.1))
    _both(r, fs, "remove_meshes", 1)
    pal70, pal3 = make_palette(70, 0.3), make_palette(3, 0.6)
    _both(r, fs, "set_mesh_pose", 1, pal70)
    _both(r, fs, "set_mesh_pose", 2, pal3)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_pose(1, pal3)                                    # (the crystal's 3-joint skin left with it)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_pose(0, pal3)
    assert r.pool_counts()["meshes"] == 3
    for w in ("indices", "mesh_infos"):
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w
    check_replica(frt, r, fs, "after remove_meshes", rebuilt=True)      # (the host scene built its tree again: the slots are compared by triangle id)


def test_multi_renderer(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    n = len(cornell_meshes(frt)[SPHERE].positions)
    skin, pal = make_skin(n, 70), make_palette(70, 0.2)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        x.set_mesh_skin(SPHERE, *skin, num_joints=70)
        x.set_mesh_pose(SPHERE, pal)
        x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    t = _up(torch, dev, pal)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_pose(SPHERE, t)
    assert frt.lib().frt_multi_renderer_set_mesh_pose(multi._h, SPHERE, t.data_ptr(), 70, frt.DEFORM_DEVICE) == -1      # the device flag on strips
    assert frt.lib().frt_multi_renderer_set_mesh_pose(multi._h, SPHERE, pal.ctypes.data, 69, 0) == -1
