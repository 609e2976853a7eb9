"""The quad walk with a copy of the tree's top (csrc/frt_trace.hpp: trace4 with `lds_top`, `lds_n`), on the host: the hits equal the brute-force loop
over all triangles whatever the size of the copy — one node, the five of the shared row, exactly the tree, more than the tree — in both forms of the
wave-uniform test (any step of the walk: the plain walk; leading steps only: the voting walk), on the Cornell Box and on a two-triangle scene whose
tree is a single node. CPU-only (tests/hostcheck/frt_top_cache_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_trace import _rays, _edge_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def tcheck(frt, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("top_cache_check") / "libfrt_top_cache_check.so")
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    flags = "-O2 -std=c++17 -fPIC --cuda-host-only -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-function".split()
    subprocess.run([HIPCC] + flags + ["-x", "hip", os.path.join(ROOT, "tests", "hostcheck", "frt_top_cache_check.cpp"), os.path.join(csrc, "frt_scene.cpp"),
                                      os.path.join(csrc, "frt_bvh.cpp"), "-shared", "-o", out], check=True)
    L = C.CDLL(out)
    L.tc_quad_nodes.restype = C.c_uint32; L.tc_quad_nodes.argtypes = [C.c_void_p]
    L.tc_trace.restype = C.c_uint32
    L.tc_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 4
    return L


def walk(L, fs, o, d, tmin, tmax, cache_n, any_hit, vote):
    n = o.shape[0]
    t = np.zeros(n, np.float32); tri = np.zeros(n, np.uint32); uv = np.zeros((n, 2), np.float32); fr = np.zeros(n, np.uint8)
    staged = L.tc_trace(fs._h, int(any_hit), int(vote), cache_n, n, o.ctypes.data, d.ctypes.data, tmin, tmax, t.ctypes.data, tri.ctypes.data, uv.ctypes.data, fr.ctypes.data)
    return staged, t, tri, uv, fr


def scenes(frt, orc, which):
    if which == "cornell":
        fs, os_ = frt.scenes.create_cornell_box(), orc.cornell()
    else:
        from _instance_lists import SceneList, two_instance_list
        from test_instance_update import oracle_scene
        base = two_instance_list(frt)
        lst = SceneList(base.meshes, base.materials, base.entries[:1])      # one plane: two triangles, one leaf
        fs = lst.build(frt)
        os_ = oracle_scene(orc, fs, lst.meshes)
    return fs, os_


@pytest.fixture(scope="module")
def rays():
    o, d = _rays(20000, 11)
    eo, ed = _edge_rays()
    return np.ascontiguousarray(np.concatenate([o, eo])), np.ascontiguousarray(np.concatenate([d, ed]))


@pytest.fixture(scope="module")
def truth(frt, orc, rays):
    """Brute force over all triangles, computed once per scene and interval."""
    out = {}
    for which in ("cornell", "two triangles"):
        fs, os_ = scenes(frt, orc, which)
        for tmin, tmax in ((0.001, 100.0), (0.0001, 0.7)):
            out[which, tmin, tmax] = (os_.trace_closest(rays[0], rays[1], tmin, tmax, False)[:4], os_.trace_any(rays[0], rays[1], tmin, tmax, False))
    return out


@pytest.mark.parametrize("vote", [False, True], ids=["re-entrant", "leading"])
@pytest.mark.parametrize("size", ["1", "5", "tree", "tree + 9"])
@pytest.mark.parametrize("which", ["cornell", "two triangles"])
def test_hits_do_not_depend_on_the_node_cache(frt, orc, tcheck, rays, truth, which, size, vote):
    fs, _ = scenes(frt, orc, which)
    nodes = tcheck.tc_quad_nodes(fs._h)
    assert nodes == (326 if which == "cornell" else 1)
    cache_n = {"1": 1, "5": 5, "tree": nodes, "tree + 9": nodes + 9}[size]
    o, d = rays
    for tmin, tmax in ((0.001, 100.0), (0.0001, 0.7)):
        (tb, ib, uvb, fb), ob = truth[which, tmin, tmax]
        staged, t, tri, uv, fr = walk(tcheck, fs, o, d, tmin, tmax, cache_n, False, vote)
        assert staged == min(cache_n, nodes)
        assert np.array_equal(tri, ib) and t.tobytes() == tb.tobytes()
        hit = ib != MISS
        assert uv[hit].tobytes() == uvb[hit].tobytes() and np.array_equal(fr[hit], fb[hit])
        if tmax > 1:
            assert hit.mean() > (0.2 if which == "cornell" else 0.01)
        _, _, tria, _, _ = walk(tcheck, fs, o, d, tmin, tmax, cache_n, True, vote)
        assert np.array_equal((tria != MISS).astype(np.uint8), ob)
