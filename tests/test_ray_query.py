"""Ray queries, host form (include/frt.h: frt_scene_trace_closest / _trace_any): the specification the device form is held to.
A hit is defined without reference to any tree, so the walk of the quad tree must equal the oracle's loop over all triangles
bit for bit, before and after instances have moved and meshes have been deformed; the record's instance / material / primitive words are checked
against the scene's own instance table. Ray families and ranges are those of test_trace.py."""
import ctypes as C
import numpy as np
import pytest
from test_trace import _rays, _edge_rays
from test_instance_update import cornell, cornell_moves, cornell_meshes, move, oracle_scene
from test_mesh_deform import deform, PLANE, SPHERE, CRYSTAL_MESH

MISS = 0xFFFFFFFF
RANGES = ((0.001, 100.0), (0.0001, 0.7))
INVALID_ARG, STATE = -1, -4


def family(which, n):
    """test_trace.py's rays: seeded random origins in the box with unit directions, plus its edge rays."""
    o, d = _rays(n, 7)
    if which == "restir":
        o = (o * np.array([5, 1, 5], np.float32)).astype(np.float32)
    eo, ed = _edge_rays()
    return np.concatenate([o, eo]), np.concatenate([d, ed])


def check_against_bruteforce(fs, os_, o, d, what=""):
    """fs.trace_closest / trace_any equal the oracle's brute force over os_; the reference's own hit share keeps the comparison from being vacuous."""
    inst, ti = fs.get("instances"), os_.get("tri_instance")
    rng = np.random.default_rng(11)
    for tmin, tmax in RANGES:
        tb, ib, uvb, fb, _ = os_.trace_closest(o, d, tmin, tmax, False)
        assert (ib != MISS).mean() > (0.2 if tmax > 1 else 0.02), what
        h = fs.trace_closest(o, d, tmin, tmax)
        hit = ib != MISS
        assert np.array_equal(h["tri"], ib), what
        assert h["t"].tobytes() == tb.tobytes(), what
        assert h["u"][hit].tobytes() == uvb[hit, 0].tobytes() and h["v"][hit].tobytes() == uvb[hit, 1].tobytes(), what
        assert np.array_equal(h["front"][hit], fb[hit].astype(np.uint32)) and set(np.unique(h["front"])) <= {0, 1}, what
        assert np.array_equal(h["instance"][hit], ti[ib[hit]]), what
        assert np.array_equal(h["material"][hit], inst[h["instance"][hit], 1]), what
        assert np.array_equal(h["primitive"][hit], ib[hit] - inst[h["instance"][hit], 2]), what
        assert np.all(h["primitive"][hit] < inst[h["instance"][hit], 3]), what
        for k in ("u", "v", "instance", "material", "primitive", "front"):      # a miss: t = -1, every other word 0
            assert not h[k][~hit].view(np.uint32).any(), (what, k)
        assert np.all(h["t"][~hit] == -1.0)
        # any-hit with a tmax of its own per ray: the oracle's, and "a closest hit exists" over the same interval
        tm = rng.uniform(tmin * 2, tmax, o.shape[0]).astype(np.float32)
        occ = fs.trace_any(o, d, tmin, tm)
        assert occ.dtype == bool and np.array_equal(occ.astype(np.uint8), os_.trace_any(o, d, tmin, tm, False)), what
        assert np.array_equal(occ, fs.trace_closest(o, d, tmin, tm)["tri"] != MISS), what
        assert np.array_equal(fs.trace_any(o, d, tmin, tmax), hit), what


def test_struct_sizes(frt):
    assert C.sizeof(frt.Ray) == 32 and C.sizeof(frt.RayHit) == 32
    assert frt.Ray.tmin.offset == 12 and frt.Ray.dir.offset == 16 and frt.Ray.tmax.offset == 28
    assert [getattr(frt.RayHit, f).offset for f in ("t", "u", "v", "tri", "instance", "material", "primitive", "front")] == list(range(0, 32, 4))


@pytest.mark.parametrize("which", ["cornell", "restir"])
def test_host_form_equals_bruteforce(frt, orc, which):
    fs = frt.scenes.create_cornell_box() if which == "cornell" else frt.scenes.create_restir_scene()
    os_ = orc.cornell() if which == "cornell" else orc.restir_scene()
    o, d = family(which, 20000 if which == "cornell" else 3000)
    check_against_bruteforce(fs, os_, o, d, which)


def test_after_moves_and_deformation(frt, orc):
    """The moves of test_instance_update.py, then three deformed meshes: each state against the oracle over a scene built from scratch in it."""
    base = cornell_meshes(frt)
    fs = cornell(frt)
    o, d = family("cornell", 4000)
    before = fs.trace_closest(o, d, 0.001, 100.0)
    move(fs, cornell_moves(frt))
    check_against_bruteforce(fs, oracle_scene(orc, fs, base), o, d, "moved")
    moved = fs.trace_closest(o, d, 0.001, 100.0)
    assert (moved["tri"] != before["tri"]).any() or moved["t"].tobytes() != before["t"].tobytes()
    meshes = list(base)
    for m in (PLANE, SPHERE, CRYSTAL_MESH):
        meshes[m] = deform(frt, base[m], 0.3 * m)
        fs.set_mesh_vertices(m, meshes[m].positions, meshes[m].attributes)
    check_against_bruteforce(fs, oracle_scene(orc, fs, meshes), o, d, "moved and deformed")
    assert fs.trace_closest(o, d, 0.001, 100.0)["t"].tobytes() != moved["t"].tobytes()


def degenerate_rays():
    """(origins, dirs, tmin, tmax) of rays that are misses by rule, each a copy of a ray that hits the back wall from the camera side."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    o = np.tile(np.array([[0.1, 0.2, 3.0]], np.float32), (12, 1)); d = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (12, 1))
    tmin = np.full(12, 0.001, np.float32); tmax = np.full(12, 100.0, np.float32)
    o[0, 0] = nan; o[1, 2] = inf; o[2, 1] = -inf
    d[3, 1] = nan; d[4, 0] = inf; d[5] = 0.0; d[6] = (-0.0, 0.0, -0.0)
    tmax[7] = nan; tmin[8] = nan
    tmin[9] = 5.0; tmax[9] = 5.0          # empty interval
    tmin[10] = 50.0; tmax[10] = 2.0       # reversed interval
    tmax[11] = -1.0
    return o, d, tmin, tmax


def test_degenerate_rays_are_misses(frt):
    fs = frt.scenes.create_cornell_box()
    good = fs.trace_closest([[0.1, 0.2, 3.0]], [[0.0, 0.0, -1.0]], 0.001, 100.0)
    assert good["tri"][0] != MISS and good["t"][0] == 4.0
    o, d, tmin, tmax = degenerate_rays()
    h = fs.trace_closest(o, d, tmin, tmax)
    assert np.all(h["tri"] == MISS) and np.all(h["t"] == -1.0)
    for k in ("u", "v", "instance", "material", "primitive", "front"):
        assert not h[k].view(np.uint32).any()
    assert not fs.trace_any(o, d, tmin, tmax).any()
    # an infinite tmax is a range like any other
    assert fs.trace_closest([[0.1, 0.2, 3.0]], [[0.0, 0.0, -1.0]], 0.0, np.inf)["t"][0] == 4.0
    # dir is used as given: t is in units of its length
    assert fs.trace_closest([[0.1, 0.2, 3.0]], [[0.0, 0.0, -2.0]], 0.001, 100.0)["t"][0] == 2.0


def test_argument_and_state_errors(frt):
    L = frt.lib()
    fs = frt.scenes.create_cornell_box()
    rays = np.zeros((4, 8), np.float32); hits = np.full((4, 8), 7, np.uint32); occ = np.full(4, 7, np.uint8)
    # n == 0: FRT_OK and nothing touched, null pointers included
    assert L.frt_scene_trace_closest(fs._h, 0, None, None) == 0 and L.frt_scene_trace_any(fs._h, 0, None, None) == 0
    assert L.frt_scene_trace_closest(fs._h, 0, rays.ctypes.data, hits.ctypes.data) == 0 and np.all(hits == 7)
    out = fs.trace_closest(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert out["tri"].shape == (0,) and fs.trace_any(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    # null pointers, a null scene, an oversized n
    assert L.frt_scene_trace_closest(fs._h, 4, None, hits.ctypes.data) == INVALID_ARG
    assert L.frt_scene_trace_closest(fs._h, 4, rays.ctypes.data, None) == INVALID_ARG
    assert L.frt_scene_trace_any(fs._h, 4, None, occ.ctypes.data) == INVALID_ARG and L.frt_scene_trace_any(fs._h, 4, rays.ctypes.data, None) == INVALID_ARG
    assert L.frt_scene_trace_closest(None, 4, rays.ctypes.data, hits.ctypes.data) == INVALID_ARG
    assert L.frt_scene_trace_closest(fs._h, (1 << 26) + 1, rays.ctypes.data, hits.ctypes.data) == INVALID_ARG
    assert L.frt_scene_trace_any(fs._h, (1 << 26) + 1, rays.ctypes.data, occ.ctypes.data) == INVALID_ARG
    assert b"2^26" in L.frt_last_error()
    assert np.all(hits == 7) and np.all(occ == 7)
    # an unbuilt scene
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.create_plane())
    assert L.frt_scene_trace_closest(b._h, 4, rays.ctypes.data, hits.ctypes.data) == STATE
    assert L.frt_scene_trace_any(b._h, 4, rays.ctypes.data, occ.ctypes.data) == STATE
    with pytest.raises(frt.FrtError, match="not built"):
        b.trace_closest([[0, 0, 3]], [[0, 0, -1]])
    # the Python side: shapes that do not pair up
    with pytest.raises(frt.FrtError):
        fs.trace_closest(np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(frt.FrtError):
        fs.trace_any(np.zeros((3, 3)), np.ones((3, 3)), tmax=np.ones(2))


def test_renderer_calls_refuse_a_null_handle_without_a_device(frt):
    L = frt.lib()
    rays = np.zeros((1, 8), np.float32); hits = np.zeros((1, 8), np.uint32); xy = np.zeros((1, 2), np.uint32)
    cam = frt.CameraController().build_uniform(4 / 3, 0, 1)
    for flags in (0, frt.QUERY_DEVICE):
        assert L.frt_renderer_trace_closest(None, 1, rays.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
        assert L.frt_renderer_trace_any(None, 1, rays.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
        assert L.frt_renderer_pick(None, C.byref(cam), 1, xy.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
        assert L.frt_multi_renderer_trace_closest(None, 1, rays.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
        assert L.frt_multi_renderer_trace_any(None, 1, rays.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
        assert L.frt_multi_renderer_pick(None, C.byref(cam), 1, xy.ctypes.data, hits.ctypes.data, flags) == INVALID_ARG
    assert L.frt_renderer_trace_closest(None, 0, None, None, 0) == INVALID_ARG
