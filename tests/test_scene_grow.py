"""New meshes, materials, texture layers and lights for a running renderer (include/frt.h: frt_renderer_add_meshes and the calls after it; DESIGN.md
section 15), without a device: the Python argument helpers refuse wrong shapes and dtypes before the library sees anything, the layer plan an importer
uses is the builder's own remapping, the new symbols are exported and declared, and the validation and layout functions run clean under a sanitiser as
a stand-alone program."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from _instance_lists import one_triangle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["add_meshes", "add_materials", "add_texture", "add_lights", "register_quad_light", "register_sphere_light"]


def test_mesh_helper_refuses_wrong_shapes_and_dtypes(frt):
    from frt.scene import mesh_add_args
    G = frt.geometry.Geometry
    tri = one_triangle(frt)
    n, recs, keep = mesh_add_args(tri)      # one mesh, or a sequence of them
    assert n == 1 and recs[0].nverts == 3 and recs[0].nidx == 3 and recs[0].pos4 == keep[0][0].ctypes.data
    assert mesh_add_args([tri, frt.geometry.create_cube()])[0] == 2 and mesh_add_args([])[0] == 0
    pos, att, idx = np.asarray(tri.positions), np.asarray(tri.attributes), np.asarray(tri.indices)
    for bad in (G(pos[:, :3], att, idx), G(pos, att[:2], idx), G(pos, att, idx.reshape(1, 3)), G(pos, att, idx.astype(np.float32)), G(pos.astype(np.int32), att, idx),
                G(pos, att, np.array([0, 1, -1])), G(pos, att.astype(np.int64), idx)):
        with pytest.raises(ValueError):
            mesh_add_args(bad)
    assert mesh_add_args(G(pos.astype(np.float64), att, idx.astype(np.int64)))[1][0].nidx == 3      # (floats to f32 and integers to u32 are conversions, not refusals)


def test_the_other_helpers_refuse_wrong_shapes_and_dtypes(frt):
    from frt.scene import material_add_args, light_add_args, texture_add_args, light_register_args
    m = frt.material_new([1, 1, 1, 1])
    assert material_add_args(m)[0] == 1 and material_add_args([m, np.frombuffer(bytes(m), np.uint32)])[1].shape == (2, 16) and material_add_args([])[0] == 0
    assert light_add_args(frt.Light())[1].shape == (1, 16)
    for call in (lambda: material_add_args([np.zeros(15, np.uint32)]), lambda: light_add_args([np.zeros(17, np.uint32)]),
                 lambda: texture_add_args("color", np.zeros((1024, 1024, 3), np.uint8)), lambda: texture_add_args("data", np.zeros((1024, 1024, 4), np.float32)),
                 lambda: texture_add_args("normal", np.zeros((1024, 1024, 4), np.uint8)), lambda: texture_add_args(2, np.zeros((1024, 1024, 4), np.uint8)),
                 lambda: light_register_args(0, np.eye(3), (1, 1, 1), 1.0), lambda: light_register_args(0, np.eye(4), (1, 1), 1.0), lambda: light_register_args(-1, np.eye(4), (1, 1, 1), 1.0)):
        with pytest.raises(ValueError):
            call()
    assert texture_add_args("data", np.zeros(1024 * 1024 * 4, np.uint8))[0] == 1


def test_layer_plan_is_the_builders_remapping(frt, tmp_path):
    from test_loader import _sphere_model
    from frt.scene import gltf_layer_plan
    path, _ = _sphere_model(tmp_path, frt)
    model = frt.loader.load_gltf(path)
    b = frt.SceneBuilder()      # three colour and three data layers to begin with
    b.add_gltf_materials(model)
    mats, color_images, data_images = gltf_layer_plan(model, 3, 3)
    assert mats.tobytes() == b.get("materials").tobytes()
    assert color_images == [0, 3] and data_images == [1, 2, 4, 0]      # first use wins: base colour and emissive; normal, occlusion, metallic-roughness, then the second material's normal map
    shifted, _, _ = gltf_layer_plan(model, 10, 20)
    assert (shifted[0][12] & 0xFFFF, shifted[0][12] >> 16) == (10, 20)


def test_new_symbols_are_exported_and_declared(frt):
    L = C.CDLL(os.path.abspath(frt._lib.LIB_PATH))
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for n in ["frt_renderer_" + x for x in NAMES] + ["frt_multi_renderer_" + x for x in NAMES] + ["frt_renderer_pool_counts", "frt_model_layer_plan"]:
        assert hasattr(L, n), f"{n} is not exported"
        assert n + "(" in header and n in frt._lib.SYMBOLS
    for cls in (frt.Renderer, frt.MultiRenderer):
        assert all(callable(getattr(cls, x)) for x in NAMES)
    assert callable(frt.Renderer.pool_counts) and callable(frt.Renderer.add_gltf)
    assert C.sizeof(frt._lib.MeshData) == 32


def test_validation_and_layout_run_clean_under_a_sanitiser(tmp_path):
    """tools/mesh_edit_hostrun.cpp: the validation functions and the host layout arithmetic of the new calls, stand-alone, with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    exe = str(tmp_path / "mesh_edit_hostrun")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "mesh_edit_hostrun.cpp"), os.path.join(csrc, "frt_scene.cpp"), os.path.join(csrc, "frt_bvh.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
