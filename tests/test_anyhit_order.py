"""An any-hit ray's node step (csrc/frt_trace.hpp: trace4<ANY = true>) enters the nearest hit child and stacks the others in slot order, without the
near-to-far sort a closest-hit ray keeps. Which triangles a ray hits does not depend on that order, so occluded / unoccluded must equal the brute-force
loop over all triangles for every ray, and the stack may not pass what the builder states for the tree — on the Cornell Box, on a one-leaf scene (a
quad tree of one node) and on a tree at the stack limit of 31, in the plain and the voting loop, with the nodes read from the tree or from a staged
copy. CPU-only (tests/hostcheck/frt_anyhit_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_trace import _rays, _edge_rays
from test_instance_update import oracle_scene
from test_lds_top_gpu import scene_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TMIN = 0.001
SCENES = {"cornell": (326, 24), "one leaf": (1, None), "stack need 31": (None, 31)}      # quad nodes, stack need (None: not pinned)


@pytest.fixture(scope="module")
def acheck(frt, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("anyhit_check") / "libfrt_anyhit_check.so")
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    flags = "-O2 -std=c++17 -fPIC --cuda-host-only -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-function".split()
    subprocess.run([HIPCC] + flags + ["-x", "hip", os.path.join(ROOT, "tests", "hostcheck", "frt_anyhit_check.cpp"), os.path.join(csrc, "frt_scene.cpp"),
                                      os.path.join(csrc, "frt_bvh.cpp"), "-shared", "-o", out], check=True)
    L = C.CDLL(out)
    L.ah_quad_nodes.restype = C.c_uint32; L.ah_quad_nodes.argtypes = [C.c_void_p]
    L.ah_stack_need.restype = C.c_uint32; L.ah_stack_need.argtypes = [C.c_void_p]
    L.ah_trace_any.restype = C.c_uint32
    L.ah_trace_any.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return L


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def ray_set(os_):
    """20k random rays at two intervals, the edge rays of test_trace.py (rays lying in an axis plane with the origin on a wall, axis-parallel rays,
    rays through shared edges and corners), rays that START on a surface of this scene, rays whose tmax lies exactly AT a triangle (the hit distance
    itself: exclusive, that triangle does not count; and the next float: it counts), and rays aimed at the chain of `stack need 31` from outside."""
    o, d = _rays(20000, 13)
    eo, ed = _edge_rays()
    tmax = np.where(np.arange(20000) % 2 == 0, 100.0, 0.7).astype(np.float32)
    os_list, ds_list, tm_list = [o, eo, eo], [d, ed, ed], [tmax, np.full(len(eo), 100.0, np.float32), np.full(len(eo), 0.7, np.float32)]
    t, tri, _, _, _ = os_.trace_closest(o[:4000], d[:4000], TMIN, 100.0, False)
    hit = tri != 0xFFFFFFFF
    if hit.any():
        ho, hd, ht = o[:4000][hit], d[:4000][hit], t[hit]
        on = (ho + hd * ht[:, None]).astype(np.float32)                   # on the surface, to rounding
        nd = _unit(np.random.default_rng(17).normal(size=on.shape))
        os_list += [on, ho, ho]; ds_list += [nd, hd, hd]
        tm_list += [np.full(len(on), 100.0, np.float32), ht, np.nextafter(ht, np.float32(np.inf))]
    rng = np.random.default_rng(19)
    k = rng.integers(0, 54, 3000)
    tgt = (np.array([0.7, 0.3, 0.5]) * (0.5 ** k)[:, None]).astype(np.float32)
    ao = rng.uniform(-0.98, 0.98, (3000, 3)).astype(np.float32)
    ad = tgt - ao
    keep = np.linalg.norm(ad, axis=1) > 1e-3
    os_list.append(ao[keep]); ds_list.append(_unit(ad[keep])); tm_list.append(np.full(int(keep.sum()), 100.0, np.float32))
    return tuple(np.ascontiguousarray(np.concatenate(x)) for x in (os_list, ds_list, tm_list))


@pytest.fixture(scope="module")
def cases(frt, orc):
    """Scene, rays and the brute-force answer, once per scene."""
    out = {}
    for which in SCENES:
        lst = scene_list(frt, which)
        fs = lst.build(frt)
        os_ = oracle_scene(orc, fs, lst.meshes)
        o, d, tmax = ray_set(os_)
        out[which] = (fs, o, d, tmax, os_.trace_any(o, d, TMIN, tmax, False))
    return out


@pytest.mark.parametrize("cached", [False, True], ids=["tree", "staged copy"])
@pytest.mark.parametrize("vote", [False, True], ids=["while-while", "voting"])
@pytest.mark.parametrize("which", list(SCENES))
def test_any_hit_walk_equals_brute_force_and_keeps_to_the_stack(acheck, cases, which, vote, cached):
    fs, o, d, tmax, want = cases[which]
    nodes, need = SCENES[which]
    stated = acheck.ah_stack_need(fs._h)
    if nodes is not None:
        assert acheck.ah_quad_nodes(fs._h) == nodes
    if need is not None:
        assert stated == need
    occ = np.zeros(len(o), np.uint8)
    deepest = acheck.ah_trace_any(fs._h, int(vote), int(cached), len(o), o.ctypes.data, d.ctypes.data, TMIN, tmax.ctypes.data, occ.ctypes.data)
    print(f"{which}: {len(o)} rays, {int(want.sum())} occluded, deepest stack {deepest} of {stated}")
    bad = np.nonzero(occ != want)[0]
    assert bad.size == 0, f"{bad.size} rays differ from brute force, first: ray {bad[0]} o {o[bad[0]]} d {d[bad[0]]} tmax {tmax[bad[0]]}"
    assert deepest <= stated
    assert 0 < want.sum() < len(o)          # both answers occur
    if which == "cornell":
        assert deepest >= 3                  # the walks do stack children
