"""Morph targets of a built scene, on the host (include/frt.h: frt_scene_set_mesh_morph_targets, frt_scene_set_mesh_morph_weights,
frt_scene_set_mesh_pose_ex; DESIGN.md section 11, "Morph targets"): a morphed scene equals, byte for byte, one given set_mesh_vertices with the float32
numpy model's positions; every morph starts from the base; morph and skin compose in glTF's order; what the calls refuse changes nothing; targets follow
remove_meshes; and the host half runs clean under a sanitiser as a stand-alone program."""
import os
import re
import subprocess
import numpy as np
import pytest
from test_instance_update import cornell_meshes
from test_mesh_deform import deform, PLANE, CUBE, SPHERE, EVERYTHING
from _skin_model import skin_model, make_skin, make_palette, scene_with_a_spare_mesh
from _morph_model import F, TARGET_COUNTS, morph_model, make_targets, make_weights, overflowing_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICA = ("tri_slots", "pair_nodes", "quad_nodes", "shade_tris", "attributes")
NEW_SYMBOLS = [p + x for p in ("frt_scene_", "frt_renderer_", "frt_multi_renderer_") for x in ("set_mesh_morph_targets", "set_mesh_morph_weights", "set_mesh_pose_ex")]


def assert_same(a, b, what):
    for w in REPLICA:
        assert a.get(w).tobytes() == b.get(w).tobytes(), f"{what}: {w}"


def test_the_model_is_float32_and_ordered():
    base = np.array([[1.0, 2.0, 3.0, 1.0], [0.5, -0.25, 0.125, 7.0]], F)
    d = np.array([[[1e-8, 0, 0], [0, 0, 0]], [[1e-8, 0, 0], [0, 0, 0]], [[-1, 0, 0], [0, 0, 0]]], F)
    out = morph_model(base, d, np.ones(3, F))
    assert out[0, 0] == 0.0      # (1 + 1e-8) + 1e-8 stays 1 in float32, then - 1: a sum in another order or a wider type gives 2e-8
    assert np.array_equal(out[1], base[1]) and np.array_equal(out[:, 3], base[:, 3])


@pytest.mark.parametrize("normals", ["recompute", "keep"])
@pytest.mark.parametrize("ntargets", TARGET_COUNTS)
@pytest.mark.parametrize("mesh", [SPHERE, PLANE, CUBE], ids=["sphere 642", "plane 4", "cube 24"])
def test_morph_equals_the_numpy_model(frt, mesh, ntargets, normals):
    base = cornell_meshes(frt)[mesh].positions
    assert len(base) == {SPHERE: 642, PLANE: 4, CUBE: 24}[mesh]
    deltas, weights = make_targets(len(base), ntargets), make_weights(ntargets, 0.5)
    assert not deltas[:, 1].any() and (ntargets == 1 or not deltas[-1].any())
    assert ntargets < 3 or (weights[0] == 0 and weights[1] < 0 and weights[2] > 1)
    fs, want = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    before = {w: fs.get(w).tobytes() for w in EVERYTHING}
    fs.set_mesh_morph_targets(mesh, deltas)
    for w in EVERYTHING:
        assert fs.get(w).tobytes() == before[w], f"binding changed {w}"
    model = morph_model(base, deltas, weights)
    assert np.isfinite(model).all() and not np.array_equal(model, base) and np.array_equal(model[:, 3], base[:, 3]) and np.array_equal(model[1], base[1])
    fs.set_mesh_morph_weights(mesh, weights, normals=normals)
    want.set_mesh_vertices(mesh, model, normals=normals)
    assert_same(fs, want, f"mesh {mesh}, {ntargets} targets, {normals}")
    assert fs.get("tri_slots").tobytes() != before["tri_slots"]
    # all weights zero: the base again, every term evaluated
    fs.set_mesh_morph_weights(mesh, np.zeros(ntargets, F), normals=normals)
    want.set_mesh_vertices(mesh, morph_model(base, deltas, np.zeros(ntargets, F)), normals=normals)
    assert_same(fs, want, "zero weights")


def test_every_morph_starts_from_the_base(frt):
    meshes = cornell_meshes(frt)
    base = meshes[SPHERE].positions
    deltas = make_targets(len(base), 3)
    a, b = make_weights(3, 0.1), make_weights(3, 0.9)
    fs, want = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    fs.set_mesh_morph_targets(SPHERE, deltas)
    fs.set_mesh_morph_weights(SPHERE, a)
    fs.set_mesh_morph_weights(SPHERE, b)
    want.set_mesh_vertices(SPHERE, morph_model(base, deltas, b), normals="recompute")
    assert_same(fs, want, "two morphs in a row")
    d = deform(frt, meshes[SPHERE], 0.4)
    fs.set_mesh_vertices(SPHERE, d.positions, d.attributes)      # allowed on a mesh with targets; the base stays
    fs.set_mesh_morph_weights(SPHERE, a, normals="keep")
    want.set_mesh_vertices(SPHERE, d.positions, d.attributes)
    want.set_mesh_vertices(SPHERE, morph_model(base, deltas, a))
    assert_same(fs, want, "a morph after set_mesh_vertices")
    # bound again now, the base is the mesh as it is: the morphed one
    morphed = morph_model(base, deltas, a)
    fs.set_mesh_morph_targets(SPHERE, deltas)
    fs.set_mesh_morph_weights(SPHERE, b, normals="keep")
    want.set_mesh_vertices(SPHERE, morph_model(morphed, deltas, b))
    assert_same(fs, want, "bound again to the morphed mesh")


@pytest.mark.parametrize("ntargets", [3, 70])
def test_morph_then_skin(frt, ntargets):
    base = cornell_meshes(frt)[SPHERE].positions
    n = len(base)
    deltas, weights = make_targets(n, ntargets), make_weights(ntargets, 0.3)
    skin, pal = make_skin(n, 70), make_palette(70, 0.4)
    fs, want, plain = (frt.scenes.create_cornell_box() for _ in range(3))
    for s in (fs, plain):
        s.set_mesh_morph_targets(SPHERE, deltas)
        s.set_mesh_skin(SPHERE, *skin, num_joints=70)
    fs.set_mesh_pose(SPHERE, pal, morph_weights=weights)
    model = skin_model(morph_model(base, deltas, weights), *skin, pal)
    assert not np.array_equal(model, skin_model(base, *skin, pal))
    want.set_mesh_vertices(SPHERE, model, normals="recompute")
    assert_same(fs, want, "morph, then skin")
    # without weights the _ex call is set_mesh_pose
    lib = frt.lib()
    assert lib.frt_scene_set_mesh_pose_ex(fs._h, SPHERE, pal.ctypes.data, 70, None, 0, frt.DEFORM_RECOMPUTE_NORMALS) == 0
    plain.set_mesh_pose(SPHERE, pal)
    assert_same(fs, plain, "set_mesh_pose_ex without weights")
    for w in EVERYTHING:
        assert fs.get(w).tobytes() == plain.get(w).tobytes(), w
    # the skin's own bind copy is not read: a skin bound to the morphed mesh and a combined pose still start from the morph base
    fs.set_mesh_morph_weights(SPHERE, weights)
    fs.set_mesh_skin(SPHERE, *skin, num_joints=70)
    fs.set_mesh_pose(SPHERE, pal, morph_weights=weights, normals="keep")
    want.set_mesh_vertices(SPHERE, morph_model(base, deltas, weights), normals="recompute")
    want.set_mesh_vertices(SPHERE, model)
    assert_same(fs, want, "the morph base, not the skin's bind pose")


def test_refusals_change_nothing(frt):
    lib = frt.lib()
    base = cornell_meshes(frt)[SPHERE].positions
    n = len(base)
    deltas, weights = make_targets(n, 3), make_weights(3)
    skin, pal = make_skin(n, 3), make_palette(3)
    fs = frt.scenes.create_cornell_box()
    before = {w: fs.get(w).tobytes() for w in EVERYTHING}

    def unchanged(what):
        for w in EVERYTHING:
            assert fs.get(w).tobytes() == before[w], f"{what}: {w}"

    def refused(call, *args, **kw):
        with pytest.raises(frt.FrtError, match="error -1"):
            getattr(fs, call)(*args, **kw)

    refused("set_mesh_morph_weights", SPHERE, weights)                      # a mesh with no targets
    # the bind call
    nan_d = deltas.copy(); nan_d[1, 5, 2] = np.nan
    inf_d = deltas.copy(); inf_d[2, 641, 0] = -np.inf
    for args in ((99, deltas), (SPHERE, deltas[:, :-1]), (PLANE, deltas), (SPHERE, deltas[:0]), (SPHERE, nan_d), (SPHERE, inf_d)):
        refused("set_mesh_morph_targets", *args)
        refused("set_mesh_morph_weights", SPHERE, weights)                  # a refused bind call has bound nothing
    one = np.zeros((1, n, 3), F)
    assert lib.frt_scene_set_mesh_morph_targets(fs._h, SPHERE, one.ctypes.data, n, 4097) == -1      # above FRT_MAX_MORPH_TARGETS (refused before a delta is read)
    assert lib.frt_scene_set_mesh_morph_targets(fs._h, SPHERE, one.ctypes.data, n, 0) == -1
    with pytest.raises(frt.FrtError):
        fs.set_mesh_morph_targets(SPHERE, deltas.reshape(3, -1))
    unchanged("refused bind calls")
    unbuilt = frt.SceneBuilder()
    unbuilt.add_mesh(cornell_meshes(frt)[PLANE])
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_morph_targets(0, make_targets(4, 1))
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_morph_weights(0, make_weights(1))
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_pose(0, make_palette(1), morph_weights=make_weights(1))
    # the morph call
    fs.set_mesh_morph_targets(SPHERE, deltas)
    unchanged("binding")
    nan_w = weights.copy(); nan_w[0] = np.nan
    inf_w = weights.copy(); inf_w[2] = np.inf
    for w in (weights[:2], make_weights(4), nan_w, inf_w):
        refused("set_mesh_morph_weights", SPHERE, w)
    refused("set_mesh_morph_weights", 99, weights)
    with pytest.raises(frt.FrtError):
        fs.set_mesh_morph_weights(SPHERE, weights.reshape(3, 1))
    with pytest.raises(frt.FrtError, match="normals must be"):
        fs.set_mesh_morph_weights(SPHERE, weights, normals="smooth")
    assert lib.frt_scene_set_mesh_morph_weights(fs._h, SPHERE, weights.ctypes.data, 3, 4) == -1                      # an unknown flag bit
    assert lib.frt_scene_set_mesh_morph_weights(fs._h, SPHERE, weights.ctypes.data, 3, frt.DEFORM_DEVICE) == -1      # a scene lives in host memory
    assert lib.frt_scene_set_mesh_morph_weights(fs._h, SPHERE, None, 3, 0) == -1
    unchanged("refused morph calls")
    # finite inputs that overflow
    big_d, big_w = overflowing_weights(n, 3)
    assert not np.isfinite(morph_model(base, big_d, big_w)).all()
    fs.set_mesh_morph_targets(SPHERE, big_d)
    refused("set_mesh_morph_weights", SPHERE, big_w)
    unchanged("an overflowing morph")
    # the combined call refuses what either part refuses
    fs.set_mesh_morph_targets(SPHERE, deltas)
    refused("set_mesh_pose", SPHERE, pal, morph_weights=weights)            # no skin
    fs.set_mesh_skin(SPHERE, *skin, num_joints=3)
    nan_m = pal.copy(); nan_m[1, 13] = np.nan
    for m, w in ((pal[:2], weights), (nan_m, weights), (pal, weights[:2]), (pal, nan_w), (pal, inf_w)):
        refused("set_mesh_pose", SPHERE, m, morph_weights=w)
    assert lib.frt_scene_set_mesh_pose_ex(fs._h, SPHERE, pal.ctypes.data, 3, None, 3, 0) == -1                       # a count without weights
    assert lib.frt_scene_set_mesh_pose_ex(fs._h, SPHERE, pal.ctypes.data, 3, weights.ctypes.data, 0, 0) == -1        # weights without a count
    assert lib.frt_scene_set_mesh_pose_ex(fs._h, SPHERE, pal.ctypes.data, 3, weights.ctypes.data, 3, 4) == -1
    assert lib.frt_scene_set_mesh_pose_ex(fs._h, SPHERE, pal.ctypes.data, 3, weights.ctypes.data, 3, frt.DEFORM_DEVICE) == -1
    fs.set_mesh_morph_targets(SPHERE, big_d)
    refused("set_mesh_pose", SPHERE, pal, morph_weights=big_w)
    unchanged("refused combined calls")
    fs.set_mesh_morph_targets(SPHERE, None)                                 # the targets leave
    refused("set_mesh_morph_weights", SPHERE, weights)
    refused("set_mesh_pose", SPHERE, pal, morph_weights=weights)
    unchanged("removing the targets")


def test_targets_follow_remove_meshes(frt):
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    want, _, _ = scene_with_a_spare_mesh(frt)
    t1, t2, t3 = make_targets(len(meshes[1].positions), 3), make_targets(len(meshes[2].positions), 70), make_targets(len(meshes[3].positions), 3, seed=1)
    fs.set_mesh_morph_targets(1, t1)
    fs.set_mesh_morph_targets(2, t2)
    fs.set_mesh_morph_targets(3, t3)
    fs.remove_meshes(1); want.remove_meshes(1)      # 2 and 3 become 1 and 2
    w70, w3 = make_weights(70, 0.3), make_weights(3, 0.6)
    fs.set_mesh_morph_weights(1, w70)
    fs.set_mesh_morph_weights(2, w3)
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_morph_weights(1, w3)            # (the crystal's three targets left with it)
    want.set_mesh_vertices(1, morph_model(meshes[2].positions, t2, w70), normals="recompute")
    want.set_mesh_vertices(2, morph_model(meshes[3].positions, t3, w3), normals="recompute")
    assert_same(fs, want, "after remove_meshes")
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_morph_weights(0, w3)            # the plane never had targets


def test_new_symbols_are_declared_and_wrapped(frt):
    with open(os.path.join(ROOT, "include", "frt.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in frt._lib.SYMBOLS
    assert re.search(r"^#define FRT_MAX_MORPH_TARGETS 4096u$", header, re.M)
    for cls in (frt.SceneBuilder, frt.Renderer, frt.MultiRenderer):
        assert all(callable(getattr(cls, x)) for x in ("set_mesh_morph_targets", "set_mesh_morph_weights"))


def test_host_half_runs_clean_under_a_sanitiser(tmp_path):
    """tools/morph_hostrun.cpp, stand-alone, with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    exe = str(tmp_path / "morph_hostrun")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + san + ["-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "morph_hostrun.cpp"), os.path.join(csrc, "frt_scene.cpp"), os.path.join(csrc, "frt_bvh.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
