"""Linear-blend skinning of a built scene, on the host (include/frt.h: frt_scene_set_mesh_skin, frt_scene_set_mesh_pose; DESIGN.md section 11,
"Skinning"): a posed scene equals, byte for byte, one given set_mesh_vertices with the float32 numpy model's positions; every pose starts from the bind
pose; what the calls refuse changes nothing; skins follow remove_meshes; and a plain C host binds and poses through the header alone."""
import os
import re
import subprocess
import numpy as np
import pytest
from test_instance_update import cornell_meshes
from test_mesh_deform import deform, PLANE, CUBE, SPHERE, EVERYTHING
from _skin_model import F, JOINT_COUNTS, skin_model, plain_transform, make_skin, make_palette, overflowing_palette, scene_with_a_spare_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICA = ("tri_slots", "pair_nodes", "quad_nodes", "shade_tris", "attributes")
NEW_SYMBOLS = ("frt_scene_set_mesh_skin", "frt_scene_set_mesh_pose", "frt_renderer_set_mesh_skin", "frt_renderer_set_mesh_pose",
               "frt_multi_renderer_set_mesh_skin", "frt_multi_renderer_set_mesh_pose")


def assert_same(a, b, what):
    for w in REPLICA:
        assert a.get(w).tobytes() == b.get(w).tobytes(), f"{what}: {w}"


@pytest.mark.parametrize("normals", ["recompute", "keep"])
@pytest.mark.parametrize("njoints", JOINT_COUNTS)
@pytest.mark.parametrize("mesh", [SPHERE, PLANE, CUBE], ids=["sphere 642", "plane 4", "cube 24"])
def test_pose_equals_the_numpy_model(frt, mesh, njoints, normals):
    bind = cornell_meshes(frt)[mesh].positions
    assert len(bind) == {SPHERE: 642, PLANE: 4, CUBE: 24}[mesh]
    joints, weights = make_skin(len(bind), njoints)
    mats = make_palette(njoints, 0.5)
    assert joints.max() == njoints - 1 and (joints[1] == joints[1, 0]).all() and (weights == 0).any() and abs(float(weights[3].sum()) - 1.2) < 1e-6
    fs, want = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    before = {w: fs.get(w).tobytes() for w in EVERYTHING}
    fs.set_mesh_skin(mesh, joints, weights, num_joints=njoints)
    for w in EVERYTHING:
        assert fs.get(w).tobytes() == before[w], f"binding changed {w}"
    model = skin_model(bind, joints, weights, mats)
    assert np.isfinite(model).all() and not np.array_equal(model, bind) and np.array_equal(model[:, 3], bind[:, 3])
    fs.set_mesh_pose(mesh, mats, normals=normals)
    want.set_mesh_vertices(mesh, model, normals=normals)
    assert_same(fs, want, f"mesh {mesh}, {njoints} joints, {normals}")
    assert fs.get("tri_slots").tobytes() != before["tri_slots"]
    if njoints == 1:      # one joint at weight 1 is a plain transform: a dropped or reordered term shows here
        one = np.zeros((len(bind), 4), F); one[:, 0] = 1.0
        plain = plain_transform(bind, mats[0])
        assert np.array_equal(skin_model(bind, joints, one, mats), plain)
        fs.set_mesh_skin(mesh, None)
        fs.set_mesh_vertices(mesh, bind, normals=normals)      # back to the bind pose, bound again with the new weights
        fs.set_mesh_skin(mesh, joints, one, num_joints=1)
        fs.set_mesh_pose(mesh, mats.reshape(1, 4, 4), normals=normals)
        want.set_mesh_vertices(mesh, bind, normals=normals)
        want.set_mesh_vertices(mesh, plain, normals=normals)
        assert_same(fs, want, "a plain transform")


def test_every_pose_starts_from_the_bind_pose(frt):
    base = cornell_meshes(frt)
    bind = base[SPHERE].positions
    joints, weights = make_skin(len(bind), 3)
    a, b = make_palette(3, 0.1), make_palette(3, 0.9)
    fs, want = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    fs.set_mesh_skin(SPHERE, joints, weights)      # (num_joints: the largest index + 1)
    fs.set_mesh_pose(SPHERE, a)
    fs.set_mesh_pose(SPHERE, b)
    want.set_mesh_vertices(SPHERE, skin_model(bind, joints, weights, b), normals="recompute")
    assert_same(fs, want, "two poses in a row")
    d = deform(frt, base[SPHERE], 0.4)
    fs.set_mesh_vertices(SPHERE, d.positions, d.attributes)      # allowed on a skinned mesh; the bind pose stays
    fs.set_mesh_pose(SPHERE, a, normals="keep")
    want.set_mesh_vertices(SPHERE, d.positions, d.attributes)
    want.set_mesh_vertices(SPHERE, skin_model(bind, joints, weights, a))
    assert_same(fs, want, "a pose after set_mesh_vertices")
    # bound again now, the bind pose is the mesh as it is: the posed one
    posed = skin_model(bind, joints, weights, a)
    fs.set_mesh_skin(SPHERE, joints, weights)
    fs.set_mesh_pose(SPHERE, b, normals="keep")
    want.set_mesh_vertices(SPHERE, skin_model(posed, joints, weights, b))
    assert_same(fs, want, "bound again to the posed mesh")


def test_refusals_change_nothing(frt):
    lib = frt.lib()
    bind = cornell_meshes(frt)[SPHERE].positions
    n = len(bind)
    joints, weights = make_skin(n, 3)
    mats = make_palette(3)
    fs = frt.scenes.create_cornell_box()
    before = {w: fs.get(w).tobytes() for w in EVERYTHING}

    def unchanged(what):
        for w in EVERYTHING:
            assert fs.get(w).tobytes() == before[w], f"{what}: {w}"

    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(SPHERE, mats)                                      # a mesh without a skin
    # the bind call
    big = joints.copy(); big[17, 2] = 3
    nan_w = weights.copy(); nan_w[5, 1] = np.nan
    inf_w = weights.copy(); inf_w[5, 1] = np.inf
    neg_w = weights.copy(); neg_w[640, 0] = -0.25
    for args in ((99, joints, weights, 3), (SPHERE, joints[:-1], weights[:-1], 3), (PLANE, joints, weights, 3), (SPHERE, joints, weights, 0),
                 (SPHERE, big, weights, 3), (SPHERE, joints, nan_w, 3), (SPHERE, joints, inf_w, 3), (SPHERE, joints, neg_w, 3)):
        with pytest.raises(frt.FrtError, match="error -1"):
            fs.set_mesh_skin(*args[:3], num_joints=args[3])
        with pytest.raises(frt.FrtError, match="error -1"):
            fs.set_mesh_pose(SPHERE, mats)                                  # a refused bind call has bound nothing
    with pytest.raises(frt.FrtError):
        fs.set_mesh_skin(SPHERE, joints.astype(np.int64) + 70000, weights)  # the range check in front of the uint16 conversion
    assert lib.frt_scene_set_mesh_skin(fs._h, SPHERE, joints.ctypes.data, None, n, 3) == -1
    unchanged("refused bind calls")
    unbuilt = frt.SceneBuilder()
    unbuilt.add_mesh(cornell_meshes(frt)[PLANE])
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_skin(0, *make_skin(4, 1))
    with pytest.raises(frt.FrtError, match="error -4"):
        unbuilt.set_mesh_pose(0, make_palette(1))
    # the pose call
    fs.set_mesh_skin(SPHERE, joints, weights, num_joints=3)
    unchanged("binding")
    nan_m = mats.copy(); nan_m[1, 13] = np.nan
    inf_m = mats.copy(); inf_m[2, 15] = np.inf                             # row 3 is not used, and still has to be finite
    for m in (mats[:2], make_palette(4), nan_m, inf_m, overflowing_palette(3)):
        with pytest.raises(frt.FrtError, match="error -1"):
            fs.set_mesh_pose(SPHERE, m)
    assert np.isfinite(overflowing_palette(3)).all() and not np.isfinite(skin_model(bind, joints, weights, overflowing_palette(3))).all()
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(99, mats)
    with pytest.raises(frt.FrtError):
        fs.set_mesh_pose(SPHERE, mats.reshape(-1, 8))
    with pytest.raises(frt.FrtError, match="normals must be"):
        fs.set_mesh_pose(SPHERE, mats, normals="smooth")
    assert lib.frt_scene_set_mesh_pose(fs._h, SPHERE, mats.ctypes.data, 3, 4) == -1                         # an unknown flag bit
    assert lib.frt_scene_set_mesh_pose(fs._h, SPHERE, mats.ctypes.data, 3, frt.DEFORM_DEVICE) == -1         # a scene lives in host memory
    assert lib.frt_scene_set_mesh_pose(fs._h, SPHERE, None, 3, 0) == -1
    unchanged("refused pose calls")
    fs.set_mesh_skin(SPHERE, None)                                          # the skin leaves
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(SPHERE, mats)
    unchanged("removing the skin")


def test_skins_follow_remove_meshes(frt):
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    want, _, _ = scene_with_a_spare_mesh(frt)
    s1, s2, s3 = make_skin(len(meshes[1].positions), 3), make_skin(len(meshes[2].positions), 70), make_skin(len(meshes[3].positions), 3, seed=1)
    fs.set_mesh_skin(1, *s1)
    fs.set_mesh_skin(2, *s2)
    fs.set_mesh_skin(3, *s3)
    fs.remove_meshes(1); want.remove_meshes(1)      # 2 and 3 become 1 and 2
    pal70, pal3 = make_palette(70, 0.3), make_palette(3, 0.6)
    fs.set_mesh_pose(1, pal70)
    fs.set_mesh_pose(2, pal3)
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(1, pal3)                   # (the crystal's 3-joint skin left with it)
    want.set_mesh_vertices(1, skin_model(meshes[2].positions, *s2, pal70), normals="recompute")
    want.set_mesh_vertices(2, skin_model(meshes[3].positions, *s3, pal3), normals="recompute")
    assert_same(fs, want, "after remove_meshes")
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(0, pal3)                   # the plane never had a skin


def test_new_symbols_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "frt.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


SRC = os.path.join(ROOT, "tests", "cabi", "frt_cabi_skin.c")
OUT = os.path.join(ROOT, "tests", "cabi", "_build", "frt_cabi_skin")
LIBDIR = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib")


def test_c_host_binds_and_poses(frt):
    """tests/cabi/frt_cabi_skin.c: plain C99 against include/frt.h and libfrt.so alone; the scene calls need no device."""
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), SRC, "-L", LIBDIR, "-lfrt",
                    f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", OUT], check=True)
    p = subprocess.run([OUT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "skin ok" in p.stdout
