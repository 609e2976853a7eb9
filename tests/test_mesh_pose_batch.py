"""Posing several meshes of a built scene in one call, on the host (include/frt.h: frt_scene_set_mesh_poses; DESIGN.md section 11, "Posing several
meshes"): a batch equals, byte for byte, the loop of single calls in the order given and a scene given set_mesh_vertices with the float32 numpy models'
positions, for skin, morph and morph-then-skin; and the batch is atomic: what refuses any mesh of it — the last one too — changes nothing."""
import os
import re
import numpy as np
import pytest
from test_instance_update import cornell_meshes
from test_mesh_deform import PLANE, CUBE, SPHERE, EVERYTHING
from _skin_model import F, skin_model, make_skin, make_palette, overflowing_palette, scene_with_a_spare_mesh
from _morph_model import morph_model, make_targets, make_weights, overflowing_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = [PLANE, CUBE, SPHERE]      # 4, 24 and 642 vertices
J, T = 3, 5                        # one palette and one weight vector for every mesh of a batch
MODES = ("skin", "morph", "morph then skin")


def everything(s):
    return {w: s.get(w).tobytes() for w in EVERYTHING}


def assert_same(a, b, what):
    ea, eb = everything(a), everything(b)
    for w in EVERYTHING:
        assert ea[w] == eb[w], f"{what}: {w}"


def bind(scene, meshes, ids, mode, seed=0):
    """Binds what `mode` needs to every mesh of `ids`; {mesh: (skin or None, deltas or None)}."""
    bound = {}
    for m in ids:
        n = len(meshes[m].positions)
        skin = make_skin(n, J, seed=seed + m) if "skin" in mode else None
        deltas = make_targets(n, T, seed=seed + m) if "morph" in mode else None
        if deltas is not None:
            scene.set_mesh_morph_targets(m, deltas)
        if skin is not None:
            scene.set_mesh_skin(m, *skin, num_joints=J)
        bound[m] = (skin, deltas)
    return bound


def inputs(mode, phase):
    return (make_palette(J, phase) if "skin" in mode else None), (make_weights(T, phase) if "morph" in mode else None)


def single(scene, m, pal, w, normals):
    if pal is None:
        scene.set_mesh_morph_weights(m, w, normals=normals)
    else:
        scene.set_mesh_pose(m, pal, normals=normals, morph_weights=w)


def model(positions, skin, deltas, pal, w):
    p = np.ascontiguousarray(positions, F)
    if w is not None:
        p = morph_model(p, deltas, w)
    if pal is not None:
        p = skin_model(p, *skin, pal)
    return p


@pytest.mark.parametrize("normals", ["recompute", "keep"])
@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_the_loop_and_the_numpy_model(frt, mode, normals):
    meshes = cornell_meshes(frt)
    assert [len(meshes[m].positions) for m in BATCH] == [4, 24, 642]
    batch, loop, want = (frt.scenes.create_cornell_box() for _ in range(3))
    before = everything(batch)
    for s in (batch, loop):
        bound = bind(s, meshes, BATCH, mode)
    pal, w = inputs(mode, 0.4)
    batch.set_mesh_poses(BATCH, pal, w, normals=normals)
    for m in BATCH:
        single(loop, m, pal, w, normals)
        p = model(meshes[m].positions, *bound[m], pal, w)
        assert np.isfinite(p).all() and not np.array_equal(p, meshes[m].positions)
        want.set_mesh_vertices(m, p, normals=normals)
    assert_same(batch, loop, f"{mode}, {normals}: batch vs loop")
    assert_same(batch, want, f"{mode}, {normals}: batch vs numpy model")
    assert batch.get("tri_slots").tobytes() != before["tri_slots"]
    # another order, a subset, and a one-mesh batch: still the loop in the order given
    pal, w = inputs(mode, 0.9)
    batch.set_mesh_poses([SPHERE, PLANE], pal, w, normals=normals)
    batch.set_mesh_poses(CUBE, pal, w, normals=normals)
    for m in (SPHERE, PLANE, CUBE):
        single(loop, m, pal, w, normals)
    assert_same(batch, loop, f"{mode}, {normals}: second batch vs loop")


def test_a_mesh_without_an_instance_is_legal(frt):
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    loop, _, _ = scene_with_a_spare_mesh(frt)
    for s in (fs, loop):
        bind(s, meshes, [1, 2, 3], "morph then skin")
    pal, w = inputs("morph then skin", 0.3)
    fs.set_mesh_poses([1, 2, 3], pal, w)
    for m in (1, 2, 3):
        loop.set_mesh_pose(m, pal, morph_weights=w)
    assert_same(fs, loop, "a spare mesh in the batch")


@pytest.mark.parametrize("mode", MODES)
def test_refusals_change_nothing(frt, mode):
    lib = frt.lib()
    meshes = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    bound = bind(fs, meshes, BATCH, mode)
    pal, w = inputs(mode, 0.2)
    fs.set_mesh_poses(BATCH, pal, w)
    before = everything(fs)

    def refused(ids, p, x, why, code="error -1"):
        with pytest.raises(frt.FrtError, match=code):
            fs.set_mesh_poses(ids, p, x)
        now = everything(fs)
        for k in EVERYTHING:
            assert now[k] == before[k], f"{why}: {k} changed"

    good_p, good_w = inputs(mode, 0.7)
    if pal is not None:
        nan_p = good_p.copy(); nan_p[J - 1, 15] = np.nan                       # row 3 is not used, and still has to be finite
        refused(BATCH, nan_p, good_w, "a non-finite palette entry")
        refused(BATCH, make_palette(J + 1), good_w, "a palette of another joint count")
        over = overflowing_palette(J)                                          # overflows on the sphere, the LAST mesh of the batch, only:
        p0 = np.zeros((4, 4), F); p0[:, 3] = 1.0                               # the plane and the cube are moved to the origin first, where it does not
        zero = {PLANE: p0, CUBE: np.tile(p0[:1], (24, 1))}
        probe = frt.scenes.create_cornell_box()
        bind(probe, meshes, BATCH, mode)
        for s in (fs, probe):
            for m in (PLANE, CUBE):
                s.set_mesh_vertices(m, zero[m])
                if "morph" in mode:
                    s.set_mesh_morph_targets(m, np.zeros((T, len(zero[m]), 3), F))
                one = np.zeros((len(zero[m]), 4), F); one[:, 0] = 1.0          # (make_skin's vertex 3 weighs 1.2 in all: 1.2 * 3e38 overflows at the origin too)
                s.set_mesh_skin(m, bound[m][0][0], one, num_joints=J)
        zw = None if good_w is None else np.zeros(T, F)
        probe.set_mesh_poses([PLANE, CUBE], over, zw)                          # (finite where the vertices sit at the origin)
        with pytest.raises(frt.FrtError, match="error -1"):
            probe.set_mesh_poses(SPHERE, over, zw)
        before = everything(fs)
        refused(BATCH, over, zw, "an overflowing pose on the last mesh")
    if w is not None:
        inf_w = good_w.copy(); inf_w[T - 1] = np.inf                           # the all-zero target
        refused(BATCH, good_p, inf_w, "a non-finite weight")
        refused(BATCH, good_p, make_weights(T + 1), "another target count")
    if mode == "morph":
        big_d, big_w = overflowing_weights(642, T)
        fs.set_mesh_morph_targets(SPHERE, big_d)
        before = everything(fs)
        refused(BATCH, None, big_w, "an overflowing morph on the last mesh")
    refused([PLANE, CUBE, PLANE], good_p, good_w, "a mesh id twice")
    refused([PLANE, 99], good_p, good_w, "a mesh id out of range")
    refused([], good_p, good_w, "an empty batch")
    refused(list(range(1025)), good_p, good_w, "more meshes than FRT_MAX_POSE_MESHES")
    refused([PLANE, CUBE, 3], good_p, good_w, "the crystal has no binding")
    with pytest.raises(frt.FrtError, match="joint_matrices, morph_weights or both"):
        fs.set_mesh_poses(BATCH)
    with pytest.raises(frt.FrtError, match="normals must be"):
        fs.set_mesh_poses(BATCH, good_p, good_w, normals="smooth")
    ids = np.array(BATCH, np.uint32)
    pp, pj = (good_p.ctypes.data, J) if good_p is not None else (None, 0)
    wp, wt = (good_w.ctypes.data, T) if good_w is not None else (None, 0)
    assert lib.frt_scene_set_mesh_poses(fs._h, 3, ids.ctypes.data, pp, pj, wp, wt, 4) == -1                      # an unknown flag bit
    assert lib.frt_scene_set_mesh_poses(fs._h, 3, ids.ctypes.data, pp, pj, wp, wt, frt.DEFORM_DEVICE) == -1      # a scene lives in host memory
    assert lib.frt_scene_set_mesh_poses(fs._h, 3, None, pp, pj, wp, wt, 0) == -1
    assert lib.frt_scene_set_mesh_poses(fs._h, 3, ids.ctypes.data, None, 0, None, 0, 0) == -1                    # neither palette nor weights
    if good_p is not None:
        assert lib.frt_scene_set_mesh_poses(fs._h, 3, ids.ctypes.data, None, J, wp, wt, 0) == -1                 # a joint count without matrices
    now = everything(fs)
    for k in EVERYTHING:
        assert now[k] == before[k], k
    if mode == "skin":                                                         # the other source's binding is missing
        refused(BATCH, good_p, make_weights(T), "no morph targets bound")
    if mode == "morph":
        refused(BATCH, make_palette(J), good_w, "no skin bound")
    unbuilt = frt.SceneBuilder()
    unbuilt.add_mesh(meshes[PLANE])
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_poses([0], make_palette(1))


def test_new_symbols_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "frt.h")) as f:
        header = f.read()
    for name in ("frt_scene_set_mesh_poses", "frt_renderer_set_mesh_poses", "frt_multi_renderer_set_mesh_poses"):
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert re.search(r"^#define FRT_MAX_POSE_MESHES 1024u$", header, re.M)
