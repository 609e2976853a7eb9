"""Ray queries on the device (include/frt.h: frt_renderer_trace_closest / _trace_any / _pick). The host form
(tests/test_ray_query.py holds it to the oracle) is the specification: the device form must give the same bytes over the whole hit array, on the
replica as it is after moves, deformations and rebuilds, for every launch shape, and must leave the renderer's frames and statistics alone.
A picked hit must be the G-buffer's hit. Renderers are 32 x 24."""
import ctypes as C
import math
import numpy as np
import pytest
from test_trace import _rays, _edge_rays
from test_instance_update import cornell, cornell_moves, cornell_meshes, oracle_scene
from test_instance_update_gpu import gpu      # noqa: F401  (the module's device fixture)
from test_mesh_deform import deform, PLANE, SPHERE, CRYSTAL_MESH
from test_tree_rebuild_gpu import _one_mesh_scene, _args
from test_ray_query import family, degenerate_rays, MISS, RANGES, INVALID_ARG

pytestmark = pytest.mark.gpu
W, H = 32, 24
FIELDS = ("t", "u", "v", "tri", "instance", "material", "primitive", "front")
VOTE_MIN_QUAD_NODES = 32768      # csrc/frt_renderer_state.hpp: kVoteMinQuadNodes — trees of at least this many quad nodes are walked by the voting loop


def words(h):
    """A hit dict as the [n, 8] words of its frt_ray_hit records."""
    return np.stack([np.asarray(h[k]).view(np.uint32) for k in FIELDS], axis=1)


def same(a, b, what=""):
    wa, wb = words(a), words(b)
    assert wa.shape == wb.shape and wa.tobytes() == wb.tobytes(), f"{what}: {int((wa != wb).any(axis=1).sum())} of {len(wa)} records differ"


def device_equals_host(r, fs, o, d, what=""):
    rng = np.random.default_rng(5)
    for tmin, tmax in RANGES:
        same(r.trace_closest(o, d, tmin, tmax), fs.trace_closest(o, d, tmin, tmax), f"{what} closest ({tmin}, {tmax})")
        tm = rng.uniform(tmin * 2, tmax, o.shape[0]).astype(np.float32)
        assert np.array_equal(r.trace_any(o, d, tmin, tm), fs.trace_any(o, d, tmin, tm)), f"{what} any ({tmin}, {tmax})"


def device_equals_bruteforce(r, os_, o, d, what=""):
    tmin, tmax = RANGES[0]
    tb, ib, uvb, fb, _ = os_.trace_closest(o, d, tmin, tmax, False)
    h = r.trace_closest(o, d, tmin, tmax)
    hit = ib != MISS
    assert hit.mean() > 0.1, what
    assert np.array_equal(h["tri"], ib) and h["t"].tobytes() == tb.tobytes(), what
    assert h["u"][hit].tobytes() == uvb[hit, 0].tobytes() and h["v"][hit].tobytes() == uvb[hit, 1].tobytes(), what
    assert np.array_equal(h["front"][hit], fb[hit].astype(np.uint32)), what
    assert np.array_equal(h["instance"][hit], os_.get("tri_instance")[ib[hit]]), what
    assert np.array_equal(r.trace_any(o, d, tmin, tmax).astype(np.uint8), os_.trace_any(o, d, tmin, tmax, False)), what


def two_spheres(frt, orc):
    """Two icosphere(6) side by side: 163,840 triangles, a quad tree on the voting side of kVoteMinQuadNodes."""
    import _scenes
    b = _scenes.DualBuilder(frt, orc)
    m = b.add_mesh(*_scenes._geo(frt, "create_sphere", 6))
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(m, mat, _scenes._mat(-0.45, 0, 0, 0.8, 0.8, 0.8))
    b.add_instance(m, mat, _scenes._mat(0.45, 0, 0, 0.8, 0.8, 0.8))
    return b.build(share_bvh=False)


@pytest.mark.parametrize("which", ["cornell", "blob82k", "two spheres"])
def test_device_equals_host_form_and_bruteforce(gpu, orc, which):
    frt = gpu
    import _scenes
    if which == "cornell":
        fs, os_ = frt.scenes.create_cornell_box(), orc.cornell()
        o, d = family("cornell", 20000)
    elif which == "blob82k":
        fs, os_ = _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6, share_bvh=False)
        o, d = family("cornell", 2000 - len(_edge_rays()[0]))
    else:
        fs, os_ = two_spheres(frt, orc)
        o, d = family("cornell", 1000 - len(_edge_rays()[0]))
    r = frt.Renderer(fs, W, H)
    nodes = r.tree_stats()["quad_nodes"]
    print(f"{which}: {nodes} quad nodes, voting walk: {nodes >= VOTE_MIN_QUAD_NODES}")
    assert (nodes >= VOTE_MIN_QUAD_NODES) == (which == "two spheres")      # one scene on each side of the threshold
    device_equals_host(r, fs, o, d, which)
    device_equals_bruteforce(r, os_, o, d, which)
    if which == "two spheres":      # the voting walk over a device-built tree, whose stack need differs from the host tree's: both are read at launch
        r.rebuild_tree()
        after = r.tree_stats()
        print(f"{which}: after rebuild_tree {after}")
        device_equals_host(r, fs, o, d, which + " rebuilt")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_ray_counts(gpu, n):
    """Partial waves, partial blocks, one lane alone: lanes past n walk a ray that cannot hit and must not disturb the others."""
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    o, d = _rays(1000, 13)
    want = fs.trace_closest(o, d, 0.001, 100.0)
    got = r.trace_closest(o[:n], d[:n], 0.001, 100.0)
    assert words(got).tobytes() == words(want)[:n].tobytes()
    assert np.array_equal(r.trace_any(o[:n], d[:n], 0.001, 100.0), (want["tri"] != MISS)[:n])
    # the output arrays are written for n records and not one byte further
    rays = frt.scene.ray_args(o[:n], d[:n], 0.001, 100.0)
    hits = np.full((n + 2, 8), 0xABABABAB, np.uint32); occ = np.full(n + 16, 0xAB, np.uint8)
    L = frt.lib()
    assert L.frt_renderer_trace_closest(r._h, n, rays.ctypes.data, hits.ctypes.data, 0) == 0
    assert L.frt_renderer_trace_any(r._h, n, rays.ctypes.data, occ.ctypes.data, 0) == 0
    assert hits[:n].tobytes() == words(want)[:n].tobytes() and np.all(hits[n:] == 0xABABABAB) and np.all(occ[n:] == 0xAB)


def test_after_moves_deformation_and_rebuilds(gpu, orc):
    """Every state of the replica against the host form over a host scene in the same state; a rebuild must change no hit."""
    frt = gpu
    base = cornell_meshes(frt)
    fs = cornell(frt)
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    o, d = family("cornell", 4000)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam)
    ids, mats = _args(cornell_moves(frt))
    r.set_instance_transforms(ids, mats); fs.set_instance_transforms(ids, mats)
    device_equals_host(r, fs, o, d, "moved")
    device_equals_bruteforce(r, oracle_scene(orc, fs, base), o, d, "moved")
    meshes = list(base)
    for m in (PLANE, SPHERE, CRYSTAL_MESH):
        meshes[m] = deform(frt, base[m], 0.3 * m)
        r.set_mesh_vertices(m, meshes[m].positions, meshes[m].attributes); fs.set_mesh_vertices(m, meshes[m].positions, meshes[m].attributes)
    device_equals_host(r, fs, o, d, "deformed")
    device_equals_bruteforce(r, oracle_scene(orc, fs, meshes), o, d, "deformed")
    before = r.trace_closest(o, d, 0.001, 100.0)
    host_tree = r.tree_stats()
    for quality in ("morton", "sah", "morton"):      # (the third one builds into the first rebuild's buffers again)
        r.rebuild_tree(quality=quality)
        st = r.tree_stats()
        print(f"rebuild_tree({quality}): {host_tree} -> {st}")
        assert st["origin"] == (2 if quality == "sah" else 1)
        same(r.trace_closest(o, d, 0.001, 100.0), before, f"rebuilt ({quality})")
        device_equals_host(r, fs, o, d, f"rebuilt ({quality})")
    r.render(cam)      # ... and a refit of the rebuilt tree
    back = frt.scenes.create_cornell_box().get("instances")[8, 5:21].view(np.float32).copy()      # the tall box, home again
    r.set_instance_transforms([8], [back]); fs.set_instance_transforms([8], [back])
    device_equals_host(r, fs, o, d, "refit after rebuild")


@pytest.mark.parametrize("which", ["one triangle", "coincident"])
def test_trees_below_the_staged_top(gpu, which):
    """A tree of fewer than kLdsTopNodes nodes has no staged top; a rebuilt one-triangle tree is a single node with no stack at all."""
    frt = gpu
    fs = _one_mesh_scene(frt, 1, True) if which == "one triangle" else _one_mesh_scene(frt, 301, False)
    r = frt.Renderer(fs, W, H)
    rng = np.random.default_rng(2)
    n = 500
    o = np.zeros((n, 3), np.float32); o[:, 2] = 1.0
    tgt = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.1, 0.3, n), np.full(n, -2.0)], axis=1)
    d = (tgt - o).astype(np.float32)
    want = fs.trace_closest(o, d, 0.0, 10.0)
    assert 0.05 < (want["tri"] != MISS).mean() < 1.0
    if which == "coincident":
        assert want["tri"][want["tri"] != MISS].max() == 0      # ties go to the smallest flattened triangle id
    same(r.trace_closest(o, d, 0.0, 10.0), want, which)
    for quality in ("morton", "sah"):
        r.rebuild_tree(quality=quality)
        print(f"{which}: rebuild_tree({quality}) -> {r.tree_stats()}")
        same(r.trace_closest(o, d, 0.0, 10.0), want, f"{which} rebuilt ({quality})")
        assert np.array_equal(r.trace_any(o, d, 0.0, 10.0), want["tri"] != MISS)


def test_degenerate_rays_among_good_ones(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    o, d = _rays(512, 21)
    tmin = np.full(512, 0.001, np.float32); tmax = np.full(512, 100.0, np.float32)
    good = r.trace_closest(o, d, tmin, tmax)
    bo, bd, btmin, btmax = degenerate_rays()
    at = np.arange(len(bo)) * 37 + 3      # scattered over the waves of both blocks
    o2, d2, tmin2, tmax2 = o.copy(), d.copy(), tmin.copy(), tmax.copy()
    o2[at], d2[at], tmin2[at], tmax2[at] = bo, bd, btmin, btmax
    got = r.trace_closest(o2, d2, tmin2, tmax2)
    same(got, fs.trace_closest(o2, d2, tmin2, tmax2), "mixed")
    keep = np.ones(512, bool); keep[at] = False
    assert words(got)[keep].tobytes() == words(good)[keep].tobytes()
    assert np.all(got["tri"][at] == MISS) and np.all(got["t"][at] == -1.0) and not words(got)[at][:, [1, 2, 4, 5, 6, 7]].any()
    occ = r.trace_any(o2, d2, tmin2, tmax2)
    assert not occ[at].any() and np.array_equal(occ[keep], (good["tri"] != MISS)[keep])


def primary_rays_f32(cam, xs, ys):
    """primary_ray of csrc/frt_shade.hpp in numpy float32, operation by operation (no fused multiply-add: numpy has none)."""
    f = np.float32
    vi = np.array(list(cam.view_inverse), f).reshape(4, 4); pi = np.array(list(cam.proj_inverse), f).reshape(4, 4)      # [column, row]
    mulv = lambda m, v: ((m[0] * v[0] + m[1] * v[1]) + m[2] * v[2]) + m[3] * v[3]
    M = np.stack([mulv(vi, pi[j]) for j in range(4)])
    ux = (xs.astype(f) + f(0.5)) / f(W); uy = (ys.astype(f) + f(0.5)) / f(H)
    nx = ux * f(2.0) - f(1.0); ny = f(1.0) - uy * f(2.0)
    one = np.ones_like(nx)
    tgt = ((M[0][None, :] * nx[:, None] + M[1][None, :] * ny[:, None]) + M[2][None, :] * one[:, None]) + M[3][None, :] * one[:, None]
    origin = vi[3, :3]
    v = tgt[:, :3] * (f(1.0) / tgt[:, 3])[:, None] - origin[None, :]
    rl = f(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return origin, v * rl[:, None]


@pytest.mark.parametrize("pose", ["default", "moved"])
def test_pick_is_the_gbuffer_hit(gpu, pose):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    ctl = frt.CameraController() if pose == "default" else frt.CameraController(position=(0.4, 0.25, 2.2), yaw=math.radians(-101.0), pitch=math.radians(-7.0))
    cam = ctl.build_uniform(W / H, 0, fs.num_lights)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    h = r.pick(cam, xy)      # between the phases of the open frame
    r.render_phases(cam, frt.PHASE_TEMPORAL | frt.PHASE_SPATIAL | frt.PHASE_POST)
    r.end_frame()
    gpos = r.read_buffer(frt.BUF_GPOS, 0).view(np.float32).reshape(H * W, 4)
    hit = h["tri"] != MISS
    assert np.array_equal(~hit, gpos[:, 3] == -1.0) and hit.mean() > 0.3
    origin, dirs = primary_rays_f32(cam, xs.ravel(), ys.ravel())
    pos = origin[None, :] + dirs * h["t"][:, None]
    assert pos[hit].astype(np.float32).tobytes() == gpos[hit, :3].tobytes()
    assert np.array_equal(h["material"][hit].astype(np.float32), gpos[hit, 3])
    # the same rays through trace_closest: the pick kernel's ray is the one the formula above gives
    same(r.trace_closest(np.tile(origin, (H * W, 1)), dirs, 0.001, 1000.0), h, "pick vs trace_closest")
    same(r.pick(cam, xy), h, "pick after the frame")
    with pytest.raises(frt.FrtError, match="outside"):
        r.pick(cam, [[3, 4], [W, 0]])
    with pytest.raises(frt.FrtError, match="outside"):
        r.pick(cam, [[0, H]])


def test_device_form_with_torch_tensors(gpu):
    frt = gpu
    import torch
    fs = cornell(frt)
    r = frt.Renderer(fs, W, H)
    dev = torch.device("cuda", 0)
    o, d = family("cornell", 3000)
    n = o.shape[0]
    rng = np.random.default_rng(9)
    tmax = rng.uniform(0.5, 100.0, n).astype(np.float32)
    to, td, tt = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(tmax).to(dev)
    want_old = fs.trace_closest(o, d, 0.001, tmax)
    ids, mats = _args(cornell_moves(frt))
    # two calls back to back, a move enqueued behind them, a third call behind the move: nothing waits in between
    a = r.trace_closest(to, td, 0.001, tt)
    b = r.trace_any(to, td, 0.001, tt)
    r.set_instance_transforms(ids, mats)
    c = r.trace_closest(to, td, 0.001, tt)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    xy = torch.tensor([[0, 0], [5, 7], [W - 1, H - 1], [W, 3], [2, H], [16, 12]], dtype=torch.int32, device=dev)
    p = r.pick(cam, xy)
    r.sync()
    fs.set_instance_transforms(ids, mats)
    want_new = fs.trace_closest(o, d, 0.001, tmax)
    assert words(want_old).tobytes() != words(want_new).tobytes()
    assert a["hits"].dtype == torch.int32 and tuple(a["hits"].shape) == (n, 8) and a["t"].dtype == torch.float32 and b.dtype == torch.bool
    assert a["hits"].cpu().numpy().view(np.uint32).tobytes() == words(want_old).tobytes()
    assert np.array_equal(b.cpu().numpy(), want_old["tri"] != MISS)
    assert c["hits"].cpu().numpy().view(np.uint32).tobytes() == words(want_new).tobytes()
    assert np.array_equal(c["t"].cpu().numpy(), want_new["t"]) and np.array_equal(c["tri"].cpu().numpy().view(np.uint32), want_new["tri"])
    same(r.trace_closest(o, d, 0.001, tmax), want_new, "host-pointer call")
    # pick: in-frame pixels equal the host-pointer call's, pixels outside the frame are misses
    pw = p["hits"].cpu().numpy().view(np.uint32)
    inside = [0, 1, 2, 5]
    assert pw[inside].tobytes() == words(r.pick(cam, xy.cpu().numpy()[inside])).tobytes()
    miss = np.array([np.float32(-1.0).view(np.uint32), 0, 0, MISS, 0, 0, 0, 0], np.uint32)
    assert np.array_equal(pw[3], miss) and np.array_equal(pw[4], miss)
    # argument checks of the device form
    L = frt.lib()
    rays = torch.zeros((4, 8), dtype=torch.float32, device=dev); hits = torch.zeros((4, 8), dtype=torch.int32, device=dev)
    assert L.frt_renderer_trace_closest(r._h, 4, rays.data_ptr() + 4, hits.data_ptr(), frt.QUERY_DEVICE) == INVALID_ARG
    assert L.frt_renderer_trace_closest(r._h, 4, rays.data_ptr(), hits.data_ptr(), 2) == INVALID_ARG
    assert L.frt_renderer_trace_closest(r._h, 4, None, hits.data_ptr(), frt.QUERY_DEVICE) == INVALID_ARG
    assert L.frt_renderer_trace_closest(r._h, (1 << 26) + 1, rays.data_ptr(), hits.data_ptr(), frt.QUERY_DEVICE) == INVALID_ARG
    assert L.frt_renderer_trace_closest(r._h, 0, None, None, frt.QUERY_DEVICE) == 0 and L.frt_renderer_trace_any(r._h, 0, None, None, 0) == 0
    assert L.frt_renderer_pick(r._h, None, 1, xy.data_ptr(), hits.data_ptr(), frt.QUERY_DEVICE) == INVALID_ARG


ALL_BUFFERS = [(b, i) for b in range(9) for i in (0, 1)]


def _frames(frt, flags, queries):
    """Eight frames of the Cornell Box, every other one issued in two halves; with `queries`, ray queries and picks before, between and behind them."""
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, flags=flags)
    o, d = _rays(1000, 4)
    xy = np.stack([np.arange(W * H) % W, np.arange(W * H) // W], axis=1)
    want = fs.trace_closest(o, d, 0.001, 100.0) if queries else None

    def ask(cam):
        if queries:
            same(r.trace_closest(o, d, 0.001, 100.0), want, "interleaved")
            r.trace_any(o, d, 0.001, 100.0)
            r.pick(cam, xy)
    for f in range(8):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        ask(cam)
        if f % 2:
            r.render_phases(cam, frt.PHASE_GBUFFER | frt.PHASE_TEMPORAL)
            ask(cam)
            r.render_phases(cam, frt.PHASE_SPATIAL | frt.PHASE_POST)
            r.end_frame()
        else:
            r.render(cam)      # (under the pipeline flag the next frame's G-buffer + T-trace now run ahead: the queries meet them in flight)
        ask(cam)
    bufs = {bi: r.read_buffer(*bi).tobytes() for bi in ALL_BUFFERS}
    return bufs, r.stats(), r.frame_count


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_queries_leave_frames_and_statistics_alone(gpu, flags):
    frt = gpu
    plain, st_plain, fc_plain = _frames(frt, flags, False)
    mixed, st_mixed, fc_mixed = _frames(frt, flags, True)
    for bi in ALL_BUFFERS:
        assert plain[bi] == mixed[bi], f"buffer {bi} differs after interleaved queries"
    assert fc_plain == fc_mixed == 8
    for k in ("rays_closest", "rays_any", "frames", "launches", "rays_stage", "halo_overflow", "queue_overflow", "speculated_frames", "discarded_speculations"):
        assert st_plain[k] == st_mixed[k], k
    if flags:
        assert st_mixed["speculated_frames"] > 0


def test_stats_are_not_touched_by_queries(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam)
    before = r.stats()
    o, d = _rays(10000, 8)
    r.trace_closest(o, d, 0.001, 100.0); r.trace_any(o, d, 0.001, 100.0); r.pick(cam, [[1, 2], [3, 4]])
    assert r.stats() == before and before["rays_closest"] > 0


def test_multi_renderer_answers_like_one_renderer(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    m = frt.MultiRenderer(fs, W, H, [0, 0])
    o, d = family("cornell", 2000)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    xy = np.stack([np.arange(W * H) % W, np.arange(W * H) // W], axis=1)
    ids, mats = _args(cornell_moves(frt))
    for state in ("created", "moved"):
        if state == "moved":
            m.render(cam); r.render(cam)
            m.set_instance_transforms(ids, mats); r.set_instance_transforms(ids, mats)
        same(m.trace_closest(o, d, 0.001, 100.0), r.trace_closest(o, d, 0.001, 100.0), state)
        assert np.array_equal(m.trace_any(o, d, 0.0001, 0.7), r.trace_any(o, d, 0.0001, 0.7))
        same(m.pick(cam, xy), r.pick(cam, xy), state + " pick")      # the full frame, though each strip renders 12 rows of it
    with pytest.raises(frt.FrtError, match="outside"):
        m.pick(cam, [[W, 0]])
    L = frt.lib()
    rays = np.zeros((1, 8), np.float32); hits = np.zeros((1, 8), np.uint32)
    assert L.frt_multi_renderer_trace_closest(m._h, 1, rays.ctypes.data, hits.ctypes.data, frt.QUERY_DEVICE) == INVALID_ARG
    assert L.frt_multi_renderer_trace_closest(m._h, 0, None, None, 0) == 0
