"""The leaf step of the quad walk (csrc/frt_trace.hpp: trace4) asks for BOTH in-line triangles at once: the second one's slot is `first + 1` under
count > 1 and `first` itself otherwise, so a single-triangle leaf reads its own slot twice and nothing behind the triangle array. Closest-hit and
any-hit must equal the brute-force loop over all triangles bit for bit (t, u, v, triangle, instance, front) on the smallest trees at which that
indexing can go wrong: one triangle (the array's first and last slot), three triangles (a pair and a single one, the single one in the last slot or
in the first), and trees built under FRT_BVH_LEAF = 3 / 4, where the loop over a leaf's further triangles runs behind the two in-line tests.
CPU-only (tests/hostcheck/frt_leaf_fetch_check.cpp: the walk reads an exact-size heap copy of the triangle array)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MISS = 0xFFFFFFFF
TMIN = 0.001
Z = -2.0


def tri(cx, half=0.1, top=0.2, z=Z):
    """One triangle facing +z: base 2 * half wide on y = 0, apex at y = top."""
    return [[cx - half, 0.0, z], [cx + half, 0.0, z], [cx, top, z]]


A, BIG = tri(0.0), tri(0.0, 0.16, 0.3)      # BIG contains A in the same plane: rays beside A hit BIG alone
# name -> (triangles in mesh order = flattened ids, FRT_BVH_LEAF or None)
SCENES = {
    "one": ([A], None),
    "three: twins + one right": ([A, A, tri(1.0)], None),            # twins: every hit of the pair is a tie, the lower id wins
    "three: twins + one left": ([A, A, tri(-1.0)], None),
    "three: one left first, small + big": ([tri(-1.0), A, BIG], None),
    "three: big + small, one right": ([BIG, A, tri(1.0)], None),     # the lower id is the one hit alone
    "leaf 3": ([tri(-1.5)] + [A, BIG, tri(0.0, 0.13, 0.25, Z - 0.01)] + [tri(1.2), tri(1.22, z=Z - 0.02)] + [tri(2.5 + 0.01 * k, z=Z - 0.01 * k) for k in range(3)], 3),
    "leaf 4": ([tri(-1.5)] + [A, BIG, tri(0.0, 0.13, 0.25, Z - 0.01)] + [tri(1.2), tri(1.22, z=Z - 0.02)] +
               [tri(2.5 + 0.01 * k, z=Z - 0.01 * k) for k in range(4)] + [tri(-3.0, z=Z - 0.01 * k) for k in range(4)], 4),
}


def build_scene(frt, name):
    """The scene of SCENES[name] (one mesh, one instance) and the meshes the oracle's own scene is made of."""
    tris, leaf = SCENES[name]
    n = len(tris)
    pos = np.ones((3 * n, 4), np.float32)
    pos[:, :3] = np.asarray(tris, np.float32).reshape(3 * n, 3)
    att = np.zeros((3 * n, 8), np.float32); att[:, 1] = 1.0
    g = frt.geometry.Geometry(pos, att, np.arange(3 * n, dtype=np.uint32))
    b = frt.SceneBuilder()
    mesh = b.add_mesh(g)
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(mesh, mat, np.eye(4, dtype=np.float32))
    return b.build(), [g]


def leaves(fs):
    """(first slot, count) of every leaf the quad tree refers to."""
    refs = np.ascontiguousarray(fs.get("quad_nodes")[:, 24:28]).view(np.uint32).ravel()
    refs = refs[(refs & 0x80000000) != 0]
    refs = refs[refs != MISS]
    return sorted({(int(r & 0xFFFFFF), int((r >> 24) & 0x7F)) for r in refs if (r >> 24) & 0x7F})


def rays(name, n=400):
    """n rays towards the triangles' plane, a quarter of them from behind (back faces): half aimed at points spread over the scene's extent, half at
    a random interior point of a triangle chosen at random, so that every triangle is aimed at by some rays. tmax per ray: half of them far behind the
    plane, half around the plane itself (t = 1 at z = Z for these directions), so that a leaf's triangles fall on both sides of the interval's end."""
    tris = np.asarray(SCENES[name][0], np.float32)
    rng = np.random.default_rng(len(name) * 131 + n)
    lo, hi = tris[:, :, 0].min() - 0.1, tris[:, :, 0].max() + 0.1
    tgt = np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.05, 0.35, n), np.full(n, Z)], axis=1)
    k = rng.integers(0, len(tris), n // 2)                       # half of the targets: inside a triangle chosen at random
    w = rng.dirichlet([1.0, 1.0, 1.0], n // 2)
    tgt[:n // 2] = (tris[k] * w[:, :, None]).sum(axis=1)
    org = np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.2, 0.4, n), np.full(n, 1.0)], axis=1)
    org[::4, 2] = -5.0
    d = tgt - org
    d /= np.abs(d[:, 2:3]) / 3.0                                  # |d.z| = 3 from z = 1; the rays from behind reach the plane at t = 1 as well
    org[::4] = tgt[::4] - d[::4]
    tmax = np.where(np.arange(n) % 2 == 0, 10.0, rng.uniform(0.99, 1.01, n)).astype(np.float32)
    return np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d, np.float32), tmax


def bind(path):
    L = C.CDLL(path)
    L.lf_trace.restype = None
    L.lf_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def lcheck_path(frt, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("leaf_fetch_check") / "libfrt_leaf_fetch_check.so")
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    flags = "-O2 -std=c++17 -fPIC --cuda-host-only -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-function".split()
    subprocess.run([HIPCC] + flags + ["-x", "hip", os.path.join(ROOT, "tests", "hostcheck", "frt_leaf_fetch_check.cpp"), os.path.join(csrc, "frt_scene.cpp"),
                                      os.path.join(csrc, "frt_bvh.cpp"), "-shared", "-o", out], check=True)
    return out


def brute_force(os_, o, d, tmax):
    """The oracle's loop over all triangles (nothing of any tree), for the per-ray tmax: the six words of a closest hit, and occluded or not."""
    n = len(o)
    want = np.zeros((n, 6), np.uint32)
    inst = os_.get("tri_instance")
    for tm in np.unique(tmax):
        m = tmax == tm
        t, tri_, uv, fr, _ = os_.trace_closest(o[m], d[m], TMIN, float(tm), False)
        hit = tri_ != MISS
        rec = np.zeros((int(m.sum()), 6), np.uint32)
        rec[:, 3] = tri_
        rec[hit, 0] = t[hit].view(np.uint32); rec[hit, 1] = uv[hit, 0].view(np.uint32); rec[hit, 2] = uv[hit, 1].view(np.uint32)
        rec[hit, 4] = inst[tri_[hit]]; rec[hit, 5] = fr[hit]
        want[m] = rec
    return want, os_.trace_any(o, d, TMIN, tmax, False)


def check_scene(frt, orc, L, name):
    """Builds SCENES[name] with the library `frt` has loaded (FRT_BVH_LEAF is the caller's business), checks the tree's leaves and holds both loops
    of the walk, closest-hit and any-hit, to the brute-force answer, which is computed once."""
    from test_instance_update import oracle_scene
    tris, leaf = SCENES[name]
    fs, meshes = build_scene(frt, name)
    o, d, tmax = rays(name)
    want, want_occ = brute_force(oracle_scene(orc, fs, meshes), o, d, tmax)
    lv = leaves(fs)
    print(f"{name}: {len(tris)} triangles, leaves (first slot, count) {lv}; {int((want[:, 3] != MISS).sum())} of {len(o)} rays hit, "
          f"{int(want_occ.sum())} occluded")
    assert sum(c for _, c in lv) == len(tris)
    if name == "one":
        assert lv == [(0, 1)]
    elif leaf is None:
        assert sorted(c for _, c in lv) == [1, 2]
        # the single triangle is the array's LAST slot where it lies to the right, its first where it lies to the left
        assert ((2, 1) in lv) == ("right" in name) and ((0, 1) in lv) == ("left" in name)
    else:
        assert max(c for _, c in lv) == leaf and min(c for _, c in lv) < 3      # the loop behind the two in-line tests runs, and not in every leaf
    for vote in (0, 1):      # the plain and the voting loop
        got = np.zeros((len(o), 6), np.uint32)
        L.lf_trace(fs._h, 0, vote, len(o), o.ctypes.data, d.ctypes.data, TMIN, tmax.ctypes.data, got.ctypes.data)
        miss = got[:, 3] == MISS
        assert np.array_equal(got[miss, 0].view(np.float32), tmax[miss])      # (a miss: t = tmax and the triangle word, nothing else is defined)
        got[miss, :3] = 0; got[miss, 4:6] = 0
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"vote {vote}: {bad.size} closest hits differ from brute force, first: ray {bad[0]} got {got[bad[0]]} want {want[bad[0]]}"
        occ = np.zeros((len(o), 6), np.uint32)
        L.lf_trace(fs._h, 1, vote, len(o), o.ctypes.data, d.ctypes.data, TMIN, tmax.ctypes.data, occ.ctypes.data)
        assert np.array_equal(occ[:, 3] != MISS, want_occ != 0), f"vote {vote}: any-hit differs from brute force"
    # the rays the cases are about
    hit_ids = set(want[want[:, 3] != MISS, 3].tolist())
    assert 0.2 < (want[:, 3] != MISS).mean() < 0.95 and 0 < want_occ.sum() < len(o)
    if name.startswith("three: twins"):
        assert hit_ids == {0, 2}                                  # equal t on both of the pair: the lower id
    if "big" in name:
        assert {tris.index(BIG), 0 if "left" in name else 2} <= hit_ids      # the big one (hit alone beside the small one) and the single one
    if leaf is not None:
        assert len(hit_ids) >= len(tris) - 3                      # triangles behind the first two of a leaf are closest hits too


@pytest.mark.parametrize("name", [n for n in SCENES if SCENES[n][1] is None])
def test_walk_equals_brute_force(frt, orc, lcheck_path, name):
    check_scene(frt, orc, bind(lcheck_path), name)


@pytest.mark.parametrize("name", [n for n in SCENES if SCENES[n][1] is not None])
def test_walk_equals_brute_force_on_wider_leaves(frt, orc, lcheck_path, name):
    """Only the experiments build of the library reads FRT_BVH_LEAF (csrc/frt_bvh.cpp), and a process loads one library: a child process builds the
    scene with it and runs check_scene — the same host instantiation of trace4 on that scene's arrays."""
    exp = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib", "libfrt_exp.so")
    if not os.path.exists(exp):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fast-raytracing-wgpu_amd"), "experiments"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, FRT_LIB=exp, FRT_BVH_LEAF=str(SCENES[name][1]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), name, lcheck_path], capture_output=True, text=True, timeout=300, env=env)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "libfrt_exp.so" in p.stdout


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "fast-raytracing-wgpu_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frt as _frt
    from _oracle import Oracle
    _frt.lib()
    print("library:", _frt._lib.LIB_PATH)
    check_scene(_frt, Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so")), bind(sys.argv[2]), sys.argv[1])
