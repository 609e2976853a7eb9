"""The staging blocks of the calls that edit or query a renderer's scene replica (csrc/frt_scene_edit.hip: Staging; DESIGN.md sections 11 and 12):
a block that is reused, then grown, then reused at a smaller size, with no host wait in between. Moves, deformations and queries of different sizes
back to back on the Cornell Box; the replica must equal the host scene after the same calls byte for byte, every query answer the host form's, and
a renderer that went through all of them must render what a renderer created over the final scene renders. Renderers are 32 x 24."""
import numpy as np
import pytest
from test_instance_update import cornell_meshes, move, CRYSTAL, TALL_BOX
from test_instance_update_gpu import gpu      # noqa: F401  (the module's device fixture)
from test_mesh_deform import deform, PLANE, SPHERE
from test_mesh_deform_gpu import REPLICA
from test_ray_query import family, MISS
from test_ray_query_gpu import same, primary_rays_f32, W, H

pytestmark = pytest.mark.gpu


def _camera(frt, fs, frame=0):
    return frt.CameraController().build_uniform(W / H, frame, fs.num_lights)


def _assert_replica(r, fs, selectors, what):
    for w in selectors:
        got, want = r.read_scene(w), fs.get(w)
        assert got.tobytes() == want.tobytes(), f"{what} {w}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"


def instance_sequence(frt, r, fs):
    """1 id, every id, 1 id, every id twice over (the later record of an id wins): on the renderer back to back, then on the host scene."""
    from frt.scenes import _T, _mul
    built = fs.get("instances")[:, 5:21].view(np.float32).reshape(-1, 4, 4).copy()
    n = len(built)

    def shifted(k, step):      # instance k as built, moved by an offset of its own
        return _mul(_T(0.01 * step * (k % 3 - 1), 0.004 * step, -0.01 * step * (k % 2)), built[k])
    calls = [{TALL_BOX: shifted(TALL_BOX, 1)}, {k: shifted(k, 2) for k in range(n)}, {CRYSTAL: shifted(CRYSTAL, 3)}]
    twice = list(range(n)) + list(range(n - 1, -1, -1))
    twice_mats = np.stack([shifted(k, 4 if at < n else 5).reshape(16) for at, k in enumerate(twice)])
    for moves in calls:
        ids = sorted(moves)
        r.set_instance_transforms(ids, np.stack([moves[k].reshape(16) for k in ids]))
    r.set_instance_transforms(twice, twice_mats)
    for moves in calls:
        move(fs, moves)
    fs.set_instance_transforms(twice, twice_mats)


def deform_sequence(frt, r, fs):
    """Plane (4 vertices) positions only, sphere with attributes, plane with attributes, sphere positions only."""
    base = cornell_meshes(frt)
    calls = [(PLANE, deform(frt, base[PLANE], 0.4), False), (SPHERE, deform(frt, base[SPHERE], 0.9), True),
             (PLANE, deform(frt, base[PLANE], 1.7), True), (SPHERE, deform(frt, base[SPHERE], 2.3), False)]
    assert len(base[PLANE].positions) == 4 and len(base[SPHERE].positions) > 64
    for x in (r, fs):
        for m, g, with_attributes in calls:
            x.set_mesh_vertices(m, g.positions, g.attributes if with_attributes else None)


def query_sequence(frt, r, fs, cam):
    """trace_closest with 1, 1,000 and 3 rays, trace_any with 65 rays and pick with 2 pixels in between: each against the host form. Returns the picked
    pixels and their hits."""
    o, d = family("cornell", 1200)
    xy = np.array([[W // 2, H // 2], [3, H - 2]], np.int64)
    origin, dirs = primary_rays_f32(cam, xy[:, 0], xy[:, 1])

    def closest(a, b):
        same(r.trace_closest(o[a:b], d[a:b], 0.001, 100.0), fs.trace_closest(o[a:b], d[a:b], 0.001, 100.0), f"trace_closest of {b - a} rays")
    closest(0, 1)
    got = r.trace_any(o[100:165], d[100:165], 0.0001, 0.7)
    assert got.shape == (65,) and np.array_equal(got, fs.trace_any(o[100:165], d[100:165], 0.0001, 0.7))
    closest(200, 1200)
    picked = r.pick(cam, xy)
    same(picked, fs.trace_closest(np.tile(origin, (2, 1)), dirs, 0.001, 1000.0), "pick")
    closest(7, 10)
    return xy, picked


def assert_picked_is_the_gbuffer_hit(frt, r, cam, xy, picked):
    """As test_ray_query_gpu.test_pick_is_the_gbuffer_hit, for the pixels of `xy`; the G-buffer is that of the last frame, rendered as frame 0 under `cam`."""
    gpos = r.read_buffer(frt.BUF_GPOS, 0).view(np.float32).reshape(H * W, 4)[xy[:, 1] * W + xy[:, 0]]
    hit = picked["tri"] != MISS
    assert hit.any() and np.array_equal(~hit, gpos[:, 3] == -1.0)
    origin, dirs = primary_rays_f32(cam, xy[:, 0], xy[:, 1])
    pos = origin[None, :] + dirs * picked["t"][:, None]
    assert pos[hit].astype(np.float32).tobytes() == gpos[hit, :3].tobytes()
    assert np.array_equal(picked["material"][hit].astype(np.float32), gpos[hit, 3])


def test_instance_records_of_growing_and_shrinking_calls(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    instance_sequence(frt, r, fs)
    _assert_replica(r, fs, ("tri_slots", "quad_nodes", "instances_dev", "lights"), "after four moves")


def test_deform_blocks_of_growing_and_shrinking_calls(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    before = r.read_scene("shade_tris").tobytes()
    deform_sequence(frt, r, fs)
    _assert_replica(r, fs, REPLICA, "after four deformations")
    assert r.read_scene("shade_tris").tobytes() != before


def test_query_blocks_of_growing_and_shrinking_calls(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H)
    cam = _camera(frt, fs)
    xy, picked = query_sequence(frt, r, fs, cam)
    r.render(cam)      # the one frame of this test: the G-buffer the picked hits are held to
    assert_picked_is_the_gbuffer_hit(frt, r, cam, xy, picked)


def test_all_three_on_one_pipelined_renderer(gpu):
    """Two frames (the second leaves a speculated frame in flight), the instance, deform and query sequences with a surface-area rebuild before the
    queries, one more frame: the pattern of test_mesh_deform_gpu.test_deform_after_a_rebuild_then_move."""
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)      # (the replica is a copy: the host scene is edited by its own calls)
    for f in range(2):
        r.render(_camera(frt, fs, f))
    instance_sequence(frt, r, fs)
    deform_sequence(frt, r, fs)
    r.rebuild_tree(quality="sah")
    assert r.tree_stats()["origin"] == 2
    cam = _camera(frt, fs)
    xy, picked = query_sequence(frt, r, fs, cam)
    for w in ("shade_tris", "instances_dev", "lights"):
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w
    r.clear()
    fresh = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(cam); fresh.render(cam)
    assert r.read_accum().tobytes() == fresh.read_accum().tobytes()
    assert_picked_is_the_gbuffer_hit(frt, r, cam, xy, picked)
    st, sf = r.stats(), fresh.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])
