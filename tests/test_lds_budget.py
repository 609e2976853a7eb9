"""The LDS a workgroup of the traced kernels may use is a parameter of the launch plan (csrc/frt_kernels.hpp: traced_lds_budget, walk_lds_plan): 32 KiB
by default, so that four traced workgroups leave a fifth of a CU's 160 KiB to one workgroup of a light kernel, 40 KiB on request, and 40 KiB as well
whenever 32 KiB could not hold a tree's stack rows, the 128 shared bytes and the kLdsTopNodes nodes every walk expects in LDS. The plan over both
budgets and the stack needs 1, 24 (the Cornell Box) and 31 (the builder's limit); 32 and 39 are past that limit and there only to see the fall-back
from both sides. Then the walk itself on the Cornell tree with the copies those plans give it — 5, 63, 127 nodes and the whole tree — closest and
any hits bit for bit against the brute-force loop over all triangles. CPU-only (tests/hostcheck/frt_lds_budget_check.cpp,
tests/hostcheck/frt_top_cache_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_trace import _rays, _edge_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MISS = 0xFFFFFFFF
KIB = 1024
TOP, SHARED, GRANULE = 5, 128, 512      # kLdsTopNodes, the shared words in bytes, the allocation granule
CORNELL_NODES, CORNELL_NEED = 326, 24


@pytest.fixture(scope="module")
def lcheck(frt, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lds_budget_check") / "libfrt_lds_budget_check.so")
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    hc = os.path.join(ROOT, "tests", "hostcheck")
    flags = "-O2 -std=c++17 -fPIC --cuda-host-only -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-function".split()
    subprocess.run([HIPCC] + flags + ["-x", "hip", os.path.join(hc, "frt_lds_budget_check.cpp"), os.path.join(hc, "frt_top_cache_check.cpp"),
                                      os.path.join(csrc, "frt_scene.cpp"), os.path.join(csrc, "frt_bvh.cpp"), "-shared", "-o", out], check=True)
    L = C.CDLL(out)
    L.lb_traced_plan.restype = None; L.lb_traced_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.lb_gbuffer_plan.restype = None; L.lb_gbuffer_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.lb_constants.restype = None; L.lb_constants.argtypes = [C.c_uint32, C.c_void_p]
    L.tc_quad_nodes.restype = C.c_uint32; L.tc_quad_nodes.argtypes = [C.c_void_p]
    L.tc_trace.restype = C.c_uint32
    L.tc_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 4
    return L


def traced_plan(L, need, nodes, want):
    out = np.zeros(4, np.uint32)
    L.lb_traced_plan(need + 1, nodes, want, out.ctypes.data)      # (wg_rows = stack need + 1: frt_renderer.hip)
    return dict(zip(("budget", "rows", "nodes", "bytes"), (int(v) for v in out)))


def test_constants(lcheck):
    c = np.zeros(7, np.uint32)
    lcheck.lb_constants(CORNELL_NEED + 1, c.ctypes.data)
    assert list(c[:6]) == [TOP, SHARED, GRANULE, 32 * KIB, 40 * KIB, 160 * KIB]
    assert c[6] == 32 * KIB      # what a renderer that is told nothing asks for
    assert 4 * c[3] + 32 * KIB <= c[5]      # four traced workgroups and 32 KiB beside them


@pytest.mark.parametrize("need", [1, 24, 31, 32, 39])
@pytest.mark.parametrize("want", [32 * KIB, 40 * KIB])
def test_plan_stays_inside_the_budget(lcheck, want, need):
    holds_top = need * KIB + SHARED + TOP * 128 <= want
    for nodes in (1, 3, TOP, 62, 63, 64, 127, 128, CORNELL_NODES, 1 << 20):
        p = traced_plan(lcheck, need, nodes, want)
        print(f"want {want // KIB} KiB, stack need {need}, {nodes} nodes: {p}")
        # the fall-back: 40 KiB exactly when the budget asked for cannot hold kLdsTopNodes nodes behind this tree's rows
        assert p["budget"] == (want if holds_top else 40 * KIB)
        assert p["rows"] == need
        used = p["rows"] * KIB + SHARED + p["nodes"] * 128
        assert used <= p["bytes"] <= p["budget"]
        assert p["bytes"] % GRANULE == 0
        assert p["nodes"] >= min(TOP, nodes)      # never below kLdsTopNodes (or the whole of a smaller tree)
        assert p["nodes"] == min(nodes, (p["budget"] - need * KIB - SHARED) // 128)      # ... and as many as fit


def test_the_figures_the_design_quotes(lcheck):
    assert traced_plan(lcheck, CORNELL_NEED, CORNELL_NODES, 32 * KIB) == {"budget": 32 * KIB, "rows": 24, "nodes": 63, "bytes": 32 * KIB}
    assert traced_plan(lcheck, CORNELL_NEED, CORNELL_NODES, 40 * KIB) == {"budget": 40 * KIB, "rows": 24, "nodes": 127, "bytes": 40 * KIB}
    assert traced_plan(lcheck, 31, CORNELL_NODES, 32 * KIB)["nodes"] == 7 and traced_plan(lcheck, 31, CORNELL_NODES, 40 * KIB)["nodes"] == 71
    assert traced_plan(lcheck, 32, CORNELL_NODES, 32 * KIB) == {"budget": 40 * KIB, "rows": 32, "nodes": 63, "bytes": 40 * KIB}
    # a one-node tree: one row to point at, the node, the allocation of two rows that the kernels' shared row expects
    assert traced_plan(lcheck, 0, 1, 32 * KIB) == {"budget": 32 * KIB, "rows": 1, "nodes": 1, "bytes": 2 * KIB}


@pytest.mark.parametrize("need", [1, 24, 31])
def test_gbuffer_workgroup_fits_beside_four_traced_ones(lcheck, need):
    g = np.zeros(4, np.uint32)
    lcheck.lb_gbuffer_plan(need + 1, CORNELL_NODES, g.ctypes.data)
    t = traced_plan(lcheck, need, CORNELL_NODES, 32 * KIB)
    print(f"stack need {need}: G-buffer budget {g[0]}, {g[2]} nodes, {g[3]} bytes; traced {t}")
    assert g[3] <= g[0] and g[3] % GRANULE == 0 and g[2] >= TOP
    assert 4 * t["bytes"] + int(g[3]) <= 160 * KIB


@pytest.fixture(scope="module")
def cornell_truth(frt, orc):
    """A few hundred rays into the Cornell Box and the brute-force answers, computed once."""
    o, d = _rays(400, 14)
    eo, ed = _edge_rays()
    o, d = np.ascontiguousarray(np.concatenate([o, eo])), np.ascontiguousarray(np.concatenate([d, ed]))
    os_ = orc.cornell()
    out = {}
    for tmin, tmax in ((0.001, 100.0), (0.0001, 0.7)):
        out[tmin, tmax] = (os_.trace_closest(o, d, tmin, tmax, False)[:4], os_.trace_any(o, d, tmin, tmax, False))
    return frt.scenes.create_cornell_box(), o, d, out


@pytest.mark.parametrize("vote", [False, True], ids=["re-entrant", "leading"])
@pytest.mark.parametrize("lds_n", [5, 63, 127, CORNELL_NODES])
def test_walk_with_the_copies_the_plans_give(lcheck, cornell_truth, lds_n, vote):
    fs, o, d, truth = cornell_truth
    assert lcheck.tc_quad_nodes(fs._h) == CORNELL_NODES and fs.tree_stats()["quad_stack_need"] == CORNELL_NEED
    n = o.shape[0]
    assert 300 <= n <= 1000
    for (tmin, tmax), ((tb, ib, uvb, fb), ob) in truth.items():
        res = {}
        for any_hit in (False, True):
            t = np.zeros(n, np.float32); tri = np.zeros(n, np.uint32); uv = np.zeros((n, 2), np.float32); fr = np.zeros(n, np.uint8)
            staged = lcheck.tc_trace(fs._h, int(any_hit), int(vote), lds_n, n, o.ctypes.data, d.ctypes.data, tmin, tmax,
                                     t.ctypes.data, tri.ctypes.data, uv.ctypes.data, fr.ctypes.data)
            assert staged == lds_n
            res[any_hit] = (t, tri, uv, fr)
        t, tri, uv, fr = res[False]
        hit = ib != MISS
        assert np.array_equal(tri, ib) and t.tobytes() == tb.tobytes()
        assert uv[hit].tobytes() == uvb[hit].tobytes() and np.array_equal(fr[hit], fb[hit])
        if tmax > 1:
            assert hit.mean() > 0.2
        assert np.array_equal((res[True][1] != MISS).astype(np.uint8), ob)
        assert 0 < ob.sum() < n
