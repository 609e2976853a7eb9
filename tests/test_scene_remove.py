"""Removing materials, meshes, lights and texture layers from a built scene (include/frt.h: frt_scene_remove_materials and the three calls after it;
DESIGN.md section 16), host forms: after every call the scene equals, on every selector of frt_scene_get, tree_stats and bvh_stats, the scene built
from scratch with the surviving builder calls; every refusal leaves the scene as it was; the checks, the id maps and the host forms run clean under a
sanitiser as a stand-alone program."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from _instance_lists import snapshot, assert_same_scene, trs
from _scene_remove_lists import Calls, solid_layer, point_light, rich

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = -1, -4
NAMES = ["remove_materials", "remove_meshes", "remove_lights", "remove_texture"]
QUAD, SPHERE = 0, 1      # lights of the Cornell Box (registered); cornell_list: meshes 0 plane, 1 cube, 2 sphere, 3 crystal, 4 one triangle; materials 0 - 5, 6 / 7 the lamps'


@pytest.fixture(scope="module")
def scene(frt):
    c = rich(frt)
    s = c.build(frt)
    n = s.counts()
    assert (n["materials"], n["lights"], n["meshes"], n["instances"]) == (11, 4, 5, 10)      # lights: 0, 1 add_light, 2 quad, 3 sphere; lamp materials 9, 10
    return c


@pytest.mark.parametrize("ids", [[0], [6], [8], [0, 6, 8], [6, 6]], ids=["first", "middle", "last unregistered", "several", "twice"])
def test_remove_materials(frt, scene, ids):
    c = scene
    if 0 in ids:      # material 0 (red) is used by the left wall: that wall goes first
        c = c.without_instances([3])
    s = c.build(frt)
    s.remove_materials(ids)
    assert_same_scene(frt, s, c.without_materials(ids).build(frt), f"remove_materials {ids}")


@pytest.mark.parametrize("ids", [[0], [3], [4], [0, 3, 4], [4, 4]], ids=["first", "middle", "last", "several", "twice"])
def test_remove_meshes(frt, scene, ids):
    made = scene._made_by(("inst", "quad", "sphere"))
    users = [k for k, j in enumerate(made) if scene.calls[j]["kind"] == "inst" and scene.calls[j]["mesh"] in ids]
    c = scene.without_instances(users)
    lamps = [k for k, j in enumerate(c._made_by(("light", "quad", "sphere"))) if c.calls[j]["kind"] in ("quad", "sphere") and c.calls[j]["mesh"] in ids]
    c = c.without_lights(lamps)      # (mesh 0 is also the quad lamp's)
    s = c.build(frt)
    s.remove_meshes(ids)
    assert_same_scene(frt, s, c.without_meshes(ids).build(frt), f"remove_meshes {ids}")


@pytest.mark.parametrize("ids", [[0], [2], [3], [0, 2, 3], [3, 3]], ids=["add_light", "quad", "sphere", "several", "twice"])
def test_remove_lights(frt, scene, ids):
    s = scene.build(frt)
    s.remove_lights(ids)
    want = scene.without_lights(ids).build(frt)
    assert_same_scene(frt, s, want, f"remove_lights {ids}")
    assert s.counts()["instances"] == 10 - len({i for i in ids if i >= 2})


@pytest.mark.parametrize("kind,layer", [(0, 3), (1, 3)])
def test_remove_texture(frt, scene, kind, layer):
    s = scene.build(frt)
    s.remove_texture(kind, layer)
    want = scene.without_texture(kind, layer).build(frt)
    assert_same_scene(frt, s, want, f"remove_texture {kind} {layer}")
    slot = s.get("materials")[7][12 if kind == 0 else 14] & 0xFFFF
    assert slot == 3      # material 7 named layer 4 of both kinds
    with pytest.raises(frt.FrtError):      # now in use
        s.remove_texture(kind, 3)


def test_removal_after_growth_and_other_edits(frt, scene):
    """Things added to a built scene, then removed, interleaved with the edits of sections 11 - 14: back to the first scene."""
    s = scene.build(frt)
    first = snapshot(frt, s)
    n = s.counts()
    m = trs(frt, (-0.3, 0.35, 0.3), 0.5, 0.4)
    s.add_material(frt.material_new([0.5, 0.5, 0.1, 1.0])); s.add_mesh(frt.geometry.create_crystal()); s.add_color_texture(solid_layer((1, 2, 3, 255)))
    s.add_light(point_light(frt, (0.0, 0.0, 0.0), 0.1, (1.0, 1.0, 1.0, 1.0)))
    s.register_quad_light(0, m, (1.0, 0.8, 0.6), 4.0)
    s.add_instance(n["meshes"], n["materials"], m)
    s.build()
    s.set_instance_transforms([n["instances"] + 1], [trs(frt, (0.2, 0.1, 0.3), 0.3)])
    s.remove_instances([n["instances"] + 1])
    s.remove_lights([n["lights"] + 1, n["lights"]])      # the registered lamp (with its instance and material) and the add_light light
    s.remove_materials([n["materials"]]); s.remove_meshes([n["meshes"]]); s.remove_texture(0, 5)
    after = snapshot(frt, s)
    for k in first:
        assert after[k] == first[k], k


def test_refusals_change_nothing(frt, scene):
    L = frt.lib()
    s = scene.build(frt)
    before = snapshot(frt, s)
    u32 = lambda *v: np.asarray(v, np.uint32)
    call = lambda name, ids: getattr(L, "frt_scene_" + name)(s._h, len(ids), ids.ctypes.data)
    assert call("remove_materials", u32(2)) == ERR_INVALID_ARG and b"still uses" in L.frt_last_error()                  # in use (white)
    assert call("remove_materials", u32(6, 9)) == ERR_INVALID_ARG and b"remove the light" in L.frt_last_error()         # the quad lamp's material
    assert call("remove_materials", u32(11)) == ERR_INVALID_ARG and call("remove_meshes", u32(5)) == ERR_INVALID_ARG and call("remove_lights", u32(4)) == ERR_INVALID_ARG
    assert call("remove_meshes", u32(4, 1)) == ERR_INVALID_ARG and b"still uses mesh 1" in L.frt_last_error()
    assert call("remove_lights", u32(0, 1)) == ERR_INVALID_ARG and b"still names light 1" in L.frt_last_error()      # material 7 names light 1
    for name in NAMES[:3]:
        assert getattr(L, "frt_scene_" + name)(s._h, 1, None) == ERR_INVALID_ARG and getattr(L, "frt_scene_" + name)(s._h, 0, None) == 0
        assert getattr(L, "frt_scene_" + name)(None, 0, None) == ERR_INVALID_ARG
    tex = L.frt_scene_remove_texture
    assert tex(s._h, 0, 4) == ERR_INVALID_ARG and b"still names" in L.frt_last_error() and tex(s._h, 1, 4) == ERR_INVALID_ARG      # material 7's base colour and metallic-roughness
    assert tex(s._h, 0, 2) == ERR_INVALID_ARG and tex(s._h, 1, 0) == ERR_INVALID_ARG and b"starts with" in L.frt_last_error()      # builder layers
    assert tex(s._h, 0, 5) == ERR_INVALID_ARG and tex(s._h, 2, 3) == ERR_INVALID_ARG and tex(None, 0, 3) == ERR_INVALID_ARG
    after = snapshot(frt, s)
    for k in before:
        assert after[k] == before[k], k
    unbuilt = frt.SceneBuilder()
    z = u32(0)
    for name in NAMES[:3]:
        assert getattr(L, "frt_scene_" + name)(unbuilt._h, 1, z.ctypes.data) == ERR_STATE
    assert tex(unbuilt._h, 0, 3) == ERR_STATE
    lamp_only = Calls([{"kind": "mesh", "geo": frt.geometry.create_plane()}, {"kind": "quad", "mesh": 0, "m": trs(frt, (0.0, 1.0, 0.0), 1.0), "color": (1, 1, 1), "intensity": 2.0}]).build(frt)
    assert L.frt_scene_remove_lights(lamp_only._h, 1, z.ctypes.data) == ERR_INVALID_ARG and b"every instance" in L.frt_last_error()


def test_new_symbols_are_exported_and_declared(frt):
    L = C.CDLL(os.path.abspath(frt._lib.LIB_PATH))
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for n in [p + x for p in ("frt_scene_", "frt_renderer_", "frt_multi_renderer_") for x in NAMES]:
        assert hasattr(L, n), f"{n} is not exported"
        assert n + "(" in header and n in frt._lib.SYMBOLS
    for cls in (frt.SceneBuilder, frt.Renderer, frt.MultiRenderer):
        assert all(callable(getattr(cls, x)) for x in NAMES)


def test_checks_maps_and_host_forms_run_clean_under_a_sanitiser(tmp_path):
    """tools/scene_remove_hostrun.cpp, stand-alone, with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    exe = str(tmp_path / "scene_remove_hostrun")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "scene_remove_hostrun.cpp"), os.path.join(csrc, "frt_scene.cpp"), os.path.join(csrc, "frt_bvh.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
