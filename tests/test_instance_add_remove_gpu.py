"""Adding and removing instances on the device (include/frt.h: frt_renderer_add_instances / _remove_instances). Hits are defined
without reference to any tree and ties go to the smaller flattened triangle id, so a replica whose triangles and ids equal those
of a freshly built scene renders that scene bit for bit, whatever tree the device made: every comparison here is bit equality, with a renderer over
the scene built from scratch with the same instance list, with the brute-force oracle over that scene, and of the replica's own records."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import oracle_scene, QUAD_LIGHT, SPHERE_LIGHT, TALL_BOX
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_tree_rebuild_gpu import _records
from _tree_check import check_tree
from _instance_lists import SceneList, cornell_list, two_instance_list, one_triangle, trs

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = -1, -4
BYTE_FOR_BYTE = ("materials", "lights", "instances_dev", "shade_tris")
CUBE, TRI = 1, 4      # meshes of cornell_list
CONFIGS = {"one stream": (0, 32, 24), "pipeline": (8, 48, 36)}      # flags, width, height


def check_replica(frt, r, fresh, what, origin=None):
    """The replica against the scene built from scratch: counts, the records that must equal byte for byte, the triangle slots as a set, and the tree."""
    want = fresh.counts()
    assert r.scene_counts() == {k: want[k] for k in ("tris", "instances", "materials", "lights")}, what
    for w in BYTE_FOR_BYTE:
        got, ref = r.read_scene(w), fresh.get(w)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}: {w}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words differ"
    slots = r.read_scene("tri_slots")
    assert _records(slots) == _records(fresh.get("tri_slots")), f"{what}: the triangle slots are not the fresh build's records"
    tree = check_tree(r.read_scene("quad_nodes"), slots)
    stats = r.tree_stats()
    assert {k: stats[k] for k in tree} == tree and tree["quad_stack_need"] <= 31 and stats["origin"] in ((1, 2) if origin is None else (origin,)), (what, stats, tree)


def check_frames(frt, orc, r, lst, fresh, cfg, what, frames=3, oracle=True):
    """`r` from a cleared state against a renderer over `fresh` (and the brute-force oracle over it): every buffer of every frame, and the ray counts."""
    flags, W, H = CONFIGS[cfg]
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=flags)
    ro = oracle_scene(orc, fresh, lst.meshes).renderer(W, H, 8, False, 16) if oracle else None      # brute force: nothing of any tree
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        for x in (r, rf) + ((ro,) if oracle else ()):
            x.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, f"{what}: edited vs fresh build")
        if oracle:
            compare_all(r.read_buffer, ro.read, f, f"{what}: edited vs brute-force oracle")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"]), what
    if oracle:
        so = ro.stats()["total"]
        assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"]), what


def renderer(frt, scene, cfg, frames=2):
    flags, W, H = CONFIGS[cfg]
    r = frt.Renderer(scene, W, H, max_depth=8, flags=flags)
    for f in range(frames):      # the edit comes between frames of a running renderer (under the pipeline: with the next frame's G-buffer + T-trace ahead)
        r.render(frt.CameraController().build_uniform(W / H, f, scene.num_lights))
    return r


def new_objects(frt):
    """A second box elsewhere in the room and a one-triangle instance (the triangle count becomes odd: the rebuild's leaves are pairs of slots)."""
    return [CUBE, TRI], [0, 1], np.stack([trs(frt, (0.45, -0.7, 0.35), 0.45, -0.3), trs(frt, (-0.3, 0.35, 0.3), 0.5, 0.4)])


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("quality", ["morton", "sah"])
def test_add(gpu, orc, quality, cfg):
    frt = gpu
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), cfg)
    me, ma, m = new_objects(frt)
    assert r.add_instances(me, ma, m, quality=quality) == 9
    after = lst.added(me, ma, m)
    fresh = after.build(frt)
    assert fresh.counts()["tris"] % 2 == 1
    check_replica(frt, r, fresh, f"add, {quality}", origin={"morton": 1, "sah": 2}[quality])
    check_frames(frt, orc, r, after, fresh, cfg, f"add, {quality}, {cfg}")


REMOVALS = {"first": [0], "middle": [4], "last": [TALL_BOX], "together": [0, 4, TALL_BOX], "mesh with other instances left, id twice": [1, 1]}


@pytest.mark.parametrize("case,quality,cfg", [("first", "morton", "pipeline"), ("middle", "sah", "one stream"), ("last", "sah", "pipeline"), ("together", "morton", "one stream"),
                                              ("together", "sah", "pipeline"), ("mesh with other instances left, id twice", "morton", "pipeline")])
def test_remove(gpu, orc, case, quality, cfg):
    frt = gpu
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), cfg)
    r.remove_instances(REMOVALS[case], quality=quality)
    after = lst.removed(REMOVALS[case])
    fresh = after.build(frt)
    check_replica(frt, r, fresh, f"remove {case}, {quality}", origin={"morton": 1, "sah": 2}[quality])
    check_frames(frt, orc, r, after, fresh, cfg, f"remove {case}, {quality}, {cfg}")


def test_growth(gpu, orc):
    """One small instance added 40 times to a 2-triangle scene (capacities grow on the way, most calls must fit), then 39 removed in shuffled order."""
    frt = gpu
    base = two_instance_list(frt)
    lst = SceneList(base.meshes + [one_triangle(frt)], base.materials, base.entries[:1])
    r = renderer(frt, lst.build(frt), "one stream", frames=1)
    assert r.scene_counts() == {"tris": 2, "instances": 1, "materials": 1, "lights": 0}
    for k in range(40):
        m = trs(frt, (-0.9 + 0.045 * k, 0.3 * np.sin(k), 0.5 + 0.01 * k), 0.2, 0.1 * k)
        assert r.add_instances(1, 0, m, quality="sah" if k % 2 else "morton") == 1 + k
        lst = lst.added(1, 0, m)
        assert r.scene_counts() == {"tris": 3 + k, "instances": 2 + k, "materials": 1, "lights": 0}
        if k in (12, 39):
            fresh = lst.build(frt)
            check_replica(frt, r, fresh, f"after {k + 1} adds")
            check_frames(frt, orc, r, lst, fresh, "one stream", f"after {k + 1} adds", frames=1, oracle=False)
    rng = np.random.default_rng(5)
    alive = 40                                                 # the added instances have ids 1 .. alive
    for step in range(39):                                     # shuffled: any of them, the first and the last included
        iid = 1 + int(rng.integers(alive))
        r.remove_instances(iid, quality="morton" if step % 2 else "sah")
        lst = lst.removed(iid)
        alive -= 1
        assert r.scene_counts() == {"tris": 2 + alive, "instances": 1 + alive, "materials": 1, "lights": 0}
    assert alive == 1
    fresh = lst.build(frt)
    check_replica(frt, r, fresh, "after 39 removals")
    check_frames(frt, orc, r, lst, fresh, "one stream", "after 39 removals", frames=2, oracle=True)


def test_smallest_scenes(gpu, orc):
    frt = gpu
    lst = SceneList([one_triangle(frt)], [frt.material_new([0.7, 0.6, 0.5, 1.0])], [{"kind": "inst", "mesh": 0, "mat": 0, "m": trs(frt, (0.0, 0.0, 0.0), 1.0)}])
    r = renderer(frt, lst.build(frt), "one stream", frames=1)
    steps = [("add", trs(frt, (0.3, 0.1, 0.5), 0.6, 0.2), "sah"), ("add", trs(frt, (-0.3, -0.1, 1.0), 0.5, -0.2), "morton"), ("remove", 1, "sah"), ("remove", 0, "morton")]
    for k, (op, arg, quality) in enumerate(steps):
        if op == "add":
            r.add_instances(0, 0, arg, quality=quality); lst = lst.added(0, 0, arg)
        else:
            r.remove_instances(arg, quality=quality); lst = lst.removed(arg)
        fresh = lst.build(frt)
        check_replica(frt, r, fresh, f"step {k}")
        if fresh.counts()["tris"] <= 2:
            assert r.tree_stats()["quad_nodes"] == 1 and r.tree_stats()["quad_stack_need"] == 0      # one leaf
        check_frames(frt, orc, r, lst, fresh, "one stream", f"step {k}", frames=1)
    assert r.scene_counts()["tris"] == 1
    zero = np.zeros(1, np.uint32)
    assert frt.lib().frt_renderer_remove_instances(r._h, 1, zero.ctypes.data, 0) == ERR_INVALID_ARG      # the last instance stays
    check_replica(frt, r, lst.build(frt), "after the refused removal")


def test_mixed_with_the_other_edits(gpu, orc):
    frt = gpu
    lst = cornell_list(frt)
    host = lst.build(frt)
    r = renderer(frt, lst.build(frt), "pipeline")
    cube = frt.geometry.create_cube()
    pos = np.array(cube.positions, np.float32); pos[:, 0] *= 1.0 + 0.3 * pos[:, 1]; pos[:, 2] *= 0.8
    att = np.array(cube.attributes, np.float32); att[:, 2:4] = att[:, 2:4] * 0.5 + 0.25; att[:, 0:2] = att[::-1, 0:2]
    m0, m1, m2 = trs(frt, (0.45, -0.7, 0.35), 0.45, -0.3), trs(frt, (0.35, -0.6, 0.45), 0.5, 0.8), trs(frt, (-0.5, 0.2, 0.4), 0.3, 0.1)
    for x in (r, host):
        assert x.add_instances(CUBE, 2, m0) == 9
        x.set_instance_transforms([9], [m1])                   # move the new instance
        x.set_mesh_vertices(CUBE, pos, att)                    # deform its mesh (the tall box's too), attributes included
        x.set_instance_materials([9], [0])
        x.remove_instances([3])                                # an older instance: the new one becomes 8
        assert x.add_instances(CUBE, 1, m2) == 9               # after the deformation: the new vertices and the new attributes
    r.rebuild_tree("morton")
    for w in BYTE_FOR_BYTE:
        assert r.read_scene(w).tobytes() == host.get(w).tobytes(), w
    assert _records(r.read_scene("tri_slots")) == _records(host.get("tri_slots"))
    check_tree(r.read_scene("quad_nodes"), r.read_scene("tri_slots"))
    after = lst.with_mesh(CUBE, frt.geometry.Geometry(pos, att, cube.indices)).added(CUBE, 0, m1).removed([3]).added(CUBE, 1, m2)
    fresh = after.build(frt)
    for w in BYTE_FOR_BYTE + ("tris",):
        assert host.get(w).tobytes() == fresh.get(w).tobytes(), f"host edits vs scratch build: {w}"
    check_frames(frt, orc, r, after, host, "pipeline", "mixed edits")


def test_queries(gpu):
    frt = gpu
    W, H = 32, 24
    lst = cornell_list(frt)
    host = lst.build(frt)
    r = frt.Renderer(lst.build(frt), W, H, max_depth=8)
    cam = frt.CameraController().build_uniform(W / H, 0, host.num_lights)
    centre = np.array([[W // 2, H // 2]], np.uint32)
    behind = r.pick(cam, centre)
    m = trs(frt, (0.0, 0.0, 1.0), 0.4, 0.3)                  # a box between the camera and the room's centre
    rng = np.random.default_rng(11)
    o = np.tile(np.array([0.0, 0.0, 2.9], np.float32), (256, 1)); d = rng.normal(size=(256, 3)).astype(np.float32); d[:, 2] = -np.abs(d[:, 2]) - 0.5

    def same_as_host(what):
        got, want = r.trace_closest(o, d), host.trace_closest(o, d)
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), f"{what}: trace_closest {k}"
        assert r.trace_any(o, d, 0.0, 2.5).tobytes() == host.trace_any(o, d, 0.0, 2.5).tobytes(), f"{what}: trace_any"
        return got

    for x in (r, host):
        x.add_instances(CUBE, 0, m)
    hit = r.pick(cam, centre)
    assert hit["instance"][0] == 9 and hit["material"][0] == 0 and hit["tri"][0] >= host.get("instances")[9][2] and hit["t"][0] < behind["t"][0]
    assert (same_as_host("after add")["instance"] == 9).any()
    for x in (r, host):
        x.remove_instances([0, 9])                               # the new box and the floor: what the pixel sees now (the tall box again) has shifted ids
    hit2 = r.pick(cam, centre)
    fresh = frt.Renderer(lst.removed([0]).build(frt), W, H, max_depth=8).pick(cam, centre)
    for k in hit2:
        assert hit2[k].tobytes() == fresh[k].tobytes(), k
    assert hit2["t"][0] > hit["t"][0] and hit2["instance"][0] == behind["instance"][0] - 1 and hit2["tri"][0] == behind["tri"][0] - 2      # the tall box, one instance and two triangles down
    got = same_as_host("after remove")
    assert got["instance"].max() <= 7 and (got["instance"] == TALL_BOX - 1).any()


def test_history_is_kept(gpu):
    frt = gpu
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "pipeline", frames=8)
    keep = lambda: [r.read_buffer(frt.BUF_ACCUM, 0).tobytes(), r.read_buffer(frt.BUF_ACCUM, 1).tobytes(), r.read_buffer(frt.BUF_RESERVOIR, 0).tobytes(), r.read_buffer(frt.BUF_RESERVOIR, 1).tobytes()]
    before, fc = keep(), r.frame_count
    assert fc == 8
    me, ma, m = new_objects(frt)
    r.add_instances(me, ma, m)
    assert r.frame_count == fc and keep() == before
    r.remove_instances([0])
    assert r.frame_count == fc and keep() == before
    r.render(frt.CameraController().build_uniform(W / H, 8, 2))      # and the sequence goes on
    assert r.frame_count == 9


def test_refusals_change_nothing(gpu):
    frt = gpu
    L = frt.lib()
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    r, twin = renderer(frt, lst.build(frt), "pipeline"), renderer(frt, lst.build(frt), "pipeline")
    what = BYTE_FOR_BYTE + ("tri_slots", "quad_nodes")
    state = lambda x: ({w: x.read_scene(w).tobytes() for w in what}, x.tree_stats(), x.scene_counts(), x.frame_count)
    u32 = lambda *v: np.asarray(v, np.uint32)
    eye = np.eye(4, dtype=np.float32).reshape(1, 16)
    flat = eye.copy(); flat[0, 0] = 0.0
    add = lambda me, ma, m, mode=1: L.frt_renderer_add_instances(r._h, len(me), me.ctypes.data, ma.ctypes.data, m.ctypes.data, mode)
    rem = lambda ids, mode=1: L.frt_renderer_remove_instances(r._h, len(ids), ids.ctypes.data, mode)
    assert rem(u32(QUAD_LIGHT)) == ERR_INVALID_ARG and rem(u32(0, SPHERE_LIGHT)) == ERR_INVALID_ARG      # registered-light instances
    assert rem(u32(9)) == ERR_INVALID_ARG and add(u32(5), u32(0), eye) == ERR_INVALID_ARG and add(u32(0), u32(8), eye) == ERR_INVALID_ARG      # ids out of range
    assert add(u32(0), u32(0), flat) == ERR_INVALID_ARG and add(u32(0, 0), u32(0, 0), np.concatenate([eye, flat])) == ERR_INVALID_ARG      # a singular matrix
    assert add(u32(0), u32(0), eye, 2) == ERR_INVALID_ARG and rem(u32(0), 7) == ERR_INVALID_ARG      # an unknown rebuild mode
    assert L.frt_renderer_add_instances(r._h, 1, None, None, None, 0) == ERR_INVALID_ARG and L.frt_renderer_add_instances(None, 0, None, None, None, 0) == ERR_INVALID_ARG
    assert L.frt_renderer_add_instances(r._h, 0, None, None, None, 0) == 9 and L.frt_renderer_remove_instances(r._h, 0, None, 0) == 0      # n == 0
    cam = frt.CameraController().build_uniform(W / H, 2, 2)
    for x in (r, twin):
        x.render_phases(cam, frt.PHASE_GBUFFER)
    assert add(u32(0), u32(0), eye) == ERR_STATE and rem(u32(0)) == ERR_STATE      # a frame is open
    assert b"frame is open" in L.frt_last_error()
    for x in (r, twin):
        x.render_phases(cam, frt.PHASE_ALL); x.end_frame()
    assert state(r) == state(twin)
    compare_all(r.read_buffer, twin.read_buffer, 2, "after the refusals")
    cam = frt.CameraController().build_uniform(W / H, 3, 2)
    r.render(cam); twin.render(cam)
    compare_all(r.read_buffer, twin.read_buffer, 3, "the frame after the refusals")
    assert r.stats()["rays_closest"] == twin.stats()["rays_closest"] and r.stats()["rays_any"] == twin.stats()["rays_any"]


def test_multi_renderer(gpu):
    frt = gpu
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    me, ma, m = new_objects(frt)
    one = frt.Renderer(lst.build(frt), W, H, max_depth=8, flags=flags)
    two = frt.MultiRenderer(lst.build(frt), W, H, [0, 0], max_depth=8, flags=flags)
    cams = [frt.CameraController().build_uniform(W / H, f, 2) for f in range(6)]

    def frames(lo, hi):
        for f in range(lo, hi):
            one.render(cams[f]); two.render(cams[f])
            for b, idx in ((frt.BUF_ACCUM, 0), (frt.BUF_ACCUM, 1), (frt.BUF_DISPLAY, 0), (frt.BUF_RAW, 0), (frt.BUF_RESERVOIR, 0), (frt.BUF_RESERVOIR, 1)):
                assert one.read_buffer(b, idx).tobytes() == two.read_buffer(b, idx).tobytes(), f"frame {f}, buffer {b}[{idx}]"

    frames(0, 2)
    assert one.add_instances(me, ma, m) == 9 and two.add_instances(me, ma, m) == 9
    frames(2, 4)
    one.remove_instances([9, 1], quality="morton"); two.remove_instances([9, 1], quality="morton")
    frames(4, 6)
    hit = two.pick(cams[5], [[W // 2, H // 2]])
    want = one.pick(cams[5], [[W // 2, H // 2]])
    assert all(hit[k].tobytes() == want[k].tobytes() for k in hit)
