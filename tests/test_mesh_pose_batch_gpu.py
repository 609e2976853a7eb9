"""Posing several meshes in one call on the device (include/frt.h: frt_renderer_set_mesh_poses; DESIGN.md section 11, "Posing several meshes"): after a
batch the replica equals the host scene bit for bit and equals a second renderer posed by the loop of single calls — on the host-built tree and on a
rebuilt one, with recomputed and with kept normals, for skin, morph and morph-then-skin; the frames equal those of a renderer over a scene built from
scratch with the numpy models' positions; device tensors give what host arrays give; the batch is atomic (a bad palette entry, a bad weight or an overflow
on the LAST mesh alone rejects all of it, counted once); what cannot be a batch is refused on the host; and a MultiRenderer's strips pose alike. Tiny
frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes, by_id
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import cornell_with, PLANE, CUBE, SPHERE
from test_mesh_deform_gpu import _three_spheres
from test_mesh_skin_gpu import torch_dev, check_replica, _replica, _up, EVERY, W, H      # noqa: F401  (torch_dev: a fixture)
from test_mesh_pose_batch import bind, inputs, single, model, J, T
from _skin_model import F, make_skin, make_palette, overflowing_palette, scene_with_a_spare_mesh
from _morph_model import make_targets, make_weights

pytestmark = pytest.mark.gpu


def _scene(frt, which):
    """(host scene, meshes, the batch). cornell: 4, 24 and 642 vertices in this order — the first wave spans three segments, the last block is partial,
    the plane has four instances. three spheres: 162 vertices (not a multiple of 64), three instances, one mirrored. spare: mesh 1 has no instance."""
    if which == "cornell":
        fs, meshes, ids = frt.scenes.create_cornell_box(), cornell_meshes(frt), [PLANE, CUBE, SPHERE]
        assert [len(meshes[m].positions) for m in ids] == [4, 24, 642] and (fs.get("instances")[:, 0] == PLANE).sum() >= 4
    elif which == "three spheres":
        (fs, meshes), ids = _three_spheres(frt), [1, 0]
        assert len(meshes[1].positions) == 162 and fs.get("instances")[:, 4].any()
    elif which == "spare":
        (fs, meshes, _), ids = scene_with_a_spare_mesh(frt), [1, 2, 3]
        assert not (fs.get("instances")[:, 0] == 1).any()
    else:                       # two meshes of the Cornell Box
        fs, meshes, ids = frt.scenes.create_cornell_box(), cornell_meshes(frt), [CUBE, SPHERE]
    return fs, meshes, ids


def _same_replicas(a, b, what, rebuilt=False):
    """Two renderers byte for byte; after each has rebuilt its own tree the slots are compared by triangle id and the trees not at all."""
    for w in ("shade_tris", "attributes", "normals") if rebuilt else EVERY:      # (a rebuild leaves no pair tree to read)
        assert a.read_scene(w).tobytes() == b.read_scene(w).tobytes(), f"{what}: {w}"
    if rebuilt:
        assert by_id(a.read_scene("tri_slots")).tobytes() == by_id(b.read_scene("tri_slots")).tobytes(), f"{what}: tri_slots"


def _batch_vs_host_and_loop(frt, which, mode, normals):
    fs, meshes, ids = _scene(frt, which)
    r, loop = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    start = r.read_scene("tri_slots").tobytes()
    for s in (r, loop, fs):
        bind(s, meshes, ids, mode)
    a, b = inputs(mode, 0.2), inputs(mode, 0.7)
    r.set_mesh_poses(ids, *a, normals=normals); r.set_mesh_poses(ids, *b, normals=normals)      # back to back, no sync: staging and scratch are reused
    fs.set_mesh_poses(ids, *a, normals=normals); fs.set_mesh_poses(ids, *b, normals=normals)
    for x in (a, b):
        for m in ids:
            single(loop, m, *x, normals)
    check_replica(frt, r, fs, f"{which}, {mode}, {normals}")      # (reading "normals" makes the pool of decoded normals: the calls below keep it up as well)
    _same_replicas(r, loop, f"{which}, {mode}, {normals}: batch vs loop")
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    c = inputs(mode, 1.3)
    r.set_mesh_poses(ids[::-1], *c, normals=normals); fs.set_mesh_poses(ids[::-1], *c, normals=normals)      # another order, now with the pool of normals
    for m in ids[::-1]:
        single(loop, m, *c, normals)
    check_replica(frt, r, fs, f"{which}, {mode}, {normals}, reversed")
    _same_replicas(r, loop, f"{which}, {mode}, {normals}, reversed: batch vs loop")
    r.rebuild_tree("sah"); loop.rebuild_tree("sah")
    d = inputs(mode, 1.7)
    r.set_mesh_poses(ids, *d, normals=normals); fs.set_mesh_poses(ids, *d, normals=normals)
    for m in ids:
        single(loop, m, *d, normals)
    check_replica(frt, r, fs, f"{which}, {mode}, {normals}, after rebuild_tree", rebuilt=True)
    _same_replicas(r, loop, f"{which}, {mode}, {normals}, after rebuild_tree: batch vs loop", rebuilt=True)
    assert r.deform_rejects() == 0 and loop.deform_rejects() == 0


@pytest.mark.parametrize("normals", ["recompute", "keep"])
@pytest.mark.parametrize("which", ["cornell", "three spheres", "spare"])
def test_replica_equals_the_host_scene_and_the_loop(gpu, which, normals):
    _batch_vs_host_and_loop(gpu, which, "skin", normals)


@pytest.mark.parametrize("normals", ["recompute", "keep"])
@pytest.mark.parametrize("mode", ["morph", "morph then skin"])
def test_morph_batches(gpu, mode, normals):
    assert T % 4      # not a multiple of the morph loop's unroll
    _batch_vs_host_and_loop(gpu, "two meshes", mode, normals)


def test_frames_equal_a_scene_built_from_scratch(gpu):
    frt = gpu
    base = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
    ids, mode = [CUBE, SPHERE], "morph then skin"
    for s in (r, fs):
        bound = bind(s, base, ids, mode)
    pal, w = inputs(mode, 0.4)
    r.set_mesh_poses(ids, pal, w); fs.set_mesh_poses(ids, pal, w)
    meshes = list(base)
    for m in ids:
        mi = fs.get("mesh_infos")[m]
        p = model(base[m].positions, *bound[m], pal, w)
        meshes[m] = frt.geometry.Geometry(p, fs.get("attributes")[mi[0]:mi[0] + len(p)].copy(), base[m].indices)
    fresh = cornell_with(frt, meshes)
    assert fresh.get("shade_tris").tobytes() == fs.get("shade_tris").tobytes()
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "a posed batch vs a build from scratch")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])


@pytest.mark.parametrize("normals", ["recompute", "keep"])
def test_device_tensors_equal_host_arrays(gpu, torch_dev, normals):
    frt = gpu
    torch, dev = torch_dev
    fs, meshes, ids = _scene(frt, "cornell")
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    a.read_scene("normals"); b.read_scene("normals")
    for r in (a, b):
        bind(r, meshes, ids, "morph then skin")
    last = _replica(b)
    for k, mode in enumerate(("skin", "morph", "morph then skin", "skin")):      # no sync between b's calls
        pal, w = inputs(mode, 0.3 + k)
        a.set_mesh_poses(ids, pal, w, normals=normals)
        b.set_mesh_poses(ids, None if pal is None else _up(torch, dev, pal).reshape(J, 4, 4), None if w is None else _up(torch, dev, w), normals=normals)
    got, want = _replica(b), _replica(a)
    for x in EVERY:
        assert got[x] == want[x], x
    assert got["tri_slots"] != last["tri_slots"] and b.deform_rejects() == 0
    pal, w = inputs("morph then skin", 0.1)
    with pytest.raises(TypeError, match="both"):
        b.set_mesh_poses(ids, _up(torch, dev, pal), w)
    with pytest.raises(TypeError, match="both"):
        b.set_mesh_poses(ids, pal, _up(torch, dev, w))


def test_a_bad_batch_is_rejected_whole_on_the_device(gpu, torch_dev):
    """Ordinary inputs that the device has to turn into one counted rejection of the whole batch: no mesh of it changes. (A joint index that is not
    below J cannot reach the kernels through the calls: every mesh's bound joint count has to equal the palette's. The overflow stands for it.)"""
    frt = gpu
    torch, dev = torch_dev
    fs, meshes, ids = _scene(frt, "cornell")
    nj = 70
    r, ref = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    origin = {PLANE: np.tile(np.array([[0, 0, 0, 1]], F), (4, 1)), CUBE: np.tile(np.array([[0, 0, 0, 1]], F), (24, 1))}
    for x in (r, ref):
        for m in ids:
            n = len(meshes[m].positions)
            joints, weights = make_skin(n, nj, seed=m)
            joints[joints == 33] = 34                                   # no vertex of any mesh names joint 33
            if m in origin:                                             # only the sphere, the LAST mesh of the batch, can overflow: the others sit at
                x.set_mesh_vertices(m, origin[m])                       # the origin under one joint of weight 1, where 3e38 * 0 + 3e38 is finite
                weights[:] = (1.0, 0.0, 0.0, 0.0)
            x.set_mesh_skin(m, joints, weights, num_joints=nj)
            x.set_mesh_morph_targets(m, make_targets(n, T, seed=m) if m not in origin else np.zeros((T, n, 3), F))
    assert r.deform_rejects() == 0
    start = _replica(r)
    good, good_w = make_palette(nj, 0.8), make_weights(T, 0.8)
    nan_unnamed = good.copy(); nan_unnamed[33, 12] = np.nan
    inf_w = good_w.copy(); inf_w[T - 1] = np.inf                        # the all-zero target
    over = overflowing_palette(nj)
    calls = [((_up(torch, dev, nan_unnamed), None), "recompute"), ((_up(torch, dev, over), None), "keep"), ((over, None), "recompute"),
             ((None, _up(torch, dev, inf_w)), "keep"), ((_up(torch, dev, good), _up(torch, dev, inf_w)), "recompute"), ((over, np.zeros(T, F)), "keep")]
    for k, (args, normals) in enumerate(calls):
        r.set_mesh_poses(ids, *args, normals=normals)
        assert r.deform_rejects() == k + 1
        now = _replica(r)
        for w in EVERY:
            assert now[w] == start[w], f"rejected batch {k}: {w} changed"
    # the overflow is the sphere's alone: the batch without it applies under the same palette
    r.set_mesh_poses([PLANE, CUBE], over, normals="keep"); ref.set_mesh_poses([PLANE, CUBE], over, normals="keep")
    assert r.deform_rejects() == len(calls)
    for m in (nan_unnamed,):                                            # the host form: refused, not counted
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_poses(ids, m)
    # a bad batch and a good one back to back, no sync: the good one applies fully, the counter moves by exactly one
    r.set_mesh_poses(ids, _up(torch, dev, nan_unnamed))
    r.set_mesh_poses(ids, _up(torch, dev, good), _up(torch, dev, good_w))
    ref.read_scene("normals")
    ref.set_mesh_poses(ids, good, good_w)
    assert r.deform_rejects() == len(calls) + 1 and ref.deform_rejects() == 0
    got, want = _replica(r), _replica(ref)
    for w in EVERY:
        assert got[w] == want[w], w
    assert got["tri_slots"] != start["tri_slots"]


def test_refusals(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    lib = frt.lib()
    fs, meshes, ids = _scene(frt, "cornell")
    r = frt.Renderer(fs, W, H)
    pal, w = inputs("morph then skin", 0.5)
    tp, tw = _up(torch, dev, pal), _up(torch, dev, w)
    start = _replica(r)
    for args in ((pal, None), (None, w), (pal, w), (tp, None), (None, tw), (tp, tw)):      # no mesh has a binding yet
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_poses(ids, *args)
    bind(r, meshes, [PLANE, CUBE], "morph then skin")
    for args in ((pal, None), (None, w), (pal, w), (tp, tw)):                              # the LAST mesh of the batch has none
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_poses(ids, *args)
    bind(r, meshes, [SPHERE], "morph then skin")
    nan_p = pal.copy(); nan_p[1, 7] = np.nan
    inf_w = w.copy(); inf_w[2] = -np.inf
    bad = [([], pal, None), (list(range(1025)), pal, None), ([PLANE, 99], pal, None), ([PLANE, CUBE, PLANE], pal, None), ([SPHERE, SPHERE], tp, tw),
           ([PLANE, 3], pal, None),                                                          # the crystal has no binding
           (ids, make_palette(J + 1), None), (ids, _up(torch, dev, make_palette(J + 1)), None), (ids, pal[:2], None),      # a wrong joint count
           (ids, None, make_weights(T + 1)), (ids, None, tw[:2].contiguous()),                                                # a wrong target count
           (ids, nan_p, None), (ids, pal, inf_w), (ids, None, inf_w),                                                         # a non-finite host entry
           (ids, tp.double(), None), (ids, tp[:, :12].contiguous(), None), (ids, tp.t().contiguous().t(), None), (ids, None, tw.reshape(T, 1))]
    for k, (i, p, x) in enumerate(bad):
        with pytest.raises(frt.FrtError):
            r.set_mesh_poses(i, p, x)
    with pytest.raises(frt.FrtError, match="joint_matrices, morph_weights or both"):
        r.set_mesh_poses(ids)
    with pytest.raises(frt.FrtError, match="normals must be"):
        r.set_mesh_poses(ids, pal, normals="smooth")
    n, i = 3, np.array(ids, np.uint32)
    call = lib.frt_renderer_set_mesh_poses
    assert call(r._h, n, i.ctypes.data, pal.ctypes.data, J, None, 0, frt.DEFORM_DEVICE) == -1        # host memory is not device memory
    assert call(r._h, n, i.ctypes.data, tp.data_ptr() + 4, J, None, 0, frt.DEFORM_DEVICE) == -1      # not 16-byte aligned
    assert call(r._h, n, i.ctypes.data, tp.data_ptr(), J, tw.data_ptr() + 2, T, frt.DEFORM_DEVICE) == -1
    assert call(r._h, n, i.ctypes.data, tp.data_ptr(), J, w.ctypes.data, T, frt.DEFORM_DEVICE) == -1  # one of each kind
    assert call(r._h, n, i.ctypes.data, None, J, None, 0, 0) == -1
    assert call(r._h, n, i.ctypes.data, None, 0, None, 0, 0) == -1                                    # neither palette nor weights
    assert call(r._h, n, None, pal.ctypes.data, J, None, 0, 0) == -1
    assert call(r._h, n, i.ctypes.data, pal.ctypes.data, J, None, 0, 4) == -1                         # an unknown flag bit
    # inside an open frame
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    assert call(r._h, n, i.ctypes.data, pal.ctypes.data, J, w.ctypes.data, T, 0) == -4
    assert call(r._h, n, i.ctypes.data, tp.data_ptr(), J, tw.data_ptr(), T, frt.DEFORM_DEVICE) == -4
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert r.deform_rejects() == 0
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], x
    r.set_mesh_poses(ids, tp, tw)                                                                      # and the good batch applies
    assert r.deform_rejects() == 0 and r.read_scene("tri_slots").tobytes() != start["tri_slots"]


def test_multi_renderer(gpu, torch_dev):
    """Two strips on one device. A strip's replica cannot be read back through the interface; what can be observed is every strip's rows of the frame,
    which equal those of a single renderer whose replica equals the host scene."""
    frt = gpu
    torch, dev = torch_dev
    fs, meshes, ids = _scene(frt, "cornell")
    mode = "morph then skin"
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one, fs):
        bind(x, meshes, ids, mode)
    for k, m in enumerate(("skin", "morph", mode)):
        pal, w = inputs(m, 0.2 + k)
        for x in (multi, one, fs):
            x.set_mesh_poses(ids, pal, w)
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), m
    check_replica(frt, one, fs, "the single renderer beside the strips")
    pal, w = inputs(mode, 0.9)
    tp, tw = _up(torch, dev, pal), _up(torch, dev, w)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_poses(ids, tp)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_poses(ids, pal, tw)
    i = np.array(ids, np.uint32)
    call = frt.lib().frt_multi_renderer_set_mesh_poses
    assert call(multi._h, 3, i.ctypes.data, tp.data_ptr(), J, tw.data_ptr(), T, frt.DEFORM_DEVICE) == -1      # the device flag on strips
    assert call(multi._h, 3, i.ctypes.data, pal.ctypes.data, J - 1, None, 0, 0) == -1
    dup = np.array([PLANE, PLANE, CUBE], np.uint32)
    assert call(multi._h, 3, dup.ctypes.data, pal.ctypes.data, J, None, 0, 0) == -1
