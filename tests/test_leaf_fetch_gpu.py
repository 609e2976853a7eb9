"""The leaf step of the quad walk on the device (csrc/frt_trace.hpp: trace4; tests/test_leaf_fetch.py holds the same lines to brute force on the host):
both in-line triangles are asked for at once, a single-triangle leaf reads its own slot twice. The tiny scenes of the host test through the ray
queries of a renderer, closest and any, against the brute-force oracle bit for bit; the Cornell Box at 64x48, depth 8, every buffer of two frames
and the ray counts against the oracle; one frame of a tree with leaves of up to four triangles (the experiments build reads FRT_BVH_LEAF)."""
import os
import subprocess

import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import oracle_scene
from test_instance_update_gpu import gpu      # noqa: F401  (the module's device fixture)
from test_experiments import _run, EXP, PKG
from test_leaf_fetch import MISS, TMIN, build_scene, leaves, rays, brute_force

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["one", "three: twins + one right", "three: one left first, small + big"])
def test_ray_queries_equal_brute_force(gpu, orc, name):
    frt = gpu
    fs, meshes = build_scene(frt, name)
    o, d, tmax = rays(name)
    want, want_occ = brute_force(oracle_scene(orc, fs, meshes), o, d, tmax)
    r = frt.Renderer(fs, 32, 24)
    print(f"{name}: leaves {leaves(fs)}, {int((want[:, 3] != MISS).sum())} of {len(o)} rays hit")
    h = r.trace_closest(o, d, TMIN, tmax)
    hit = want[:, 3] != MISS
    assert 0.2 < hit.mean() < 0.95
    assert np.array_equal(h["tri"], want[:, 3])
    got = np.stack([h["t"].view(np.uint32), h["u"].view(np.uint32), h["v"].view(np.uint32), h["tri"], h["instance"], h["front"].astype(np.uint32)], axis=1)
    bad = np.nonzero((got[hit] != want[hit]).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} closest hits differ from brute force, first: got {got[hit][bad[0]]} want {want[hit][bad[0]]}"
    assert np.array_equal(np.asarray(r.trace_any(o, d, TMIN, tmax)).astype(np.uint8), want_occ)


def test_cornell_frames_equal_the_oracle(gpu, orc):
    frt = gpu
    W, H = 64, 48
    fs = frt.scenes.create_cornell_box()
    os_ = orc.cornell()
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    r = frt.Renderer(fs, W, H, max_depth=8)
    ro = os_.renderer(W, H, 8, True, 16)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        r.render(cam); ro.render(cam)
        compare_all(r.read_buffer, ro.read, f, "cornell 64x48")
    st, so = r.stats(), ro.stats()["total"]
    assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"])


def test_frame_of_a_tree_with_four_triangle_leaves(gpu):
    """32x32, one frame, every buffer and the ray counts against the oracle, in a child process that loads the experiments build."""
    frt = gpu
    if not os.path.exists(EXP):
        subprocess.run(["make", "-C", PKG, "experiments"], check=True, stdout=subprocess.DEVNULL)
    res = _run({"FRT_BVH_LEAF": "4"}, 0, args=("cornell", 32, 32, 8, 1))
    assert res["ok"] and res["lib"].endswith("libfrt_exp.so"), res
