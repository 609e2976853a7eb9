"""Animating a cast on the device (include/frt.h: frt_renderer_animate_cast; DESIGN.md section 11, "Animating a cast"): after one animate_cast the
replica, the bindings' own buffers and the frames equal, bit for bit, those of a renderer given the same entries through animate_instances and animate
one by one — for one entry of either kind and for five mixed entries with three different rigs whose small meshes share a wave of the pose kernels;
a character on an instance the same call moves takes the moved matrix from the device table; the halves reject on their own; what the header says is
refused is refused with nothing changed; bindings follow removals; set_mesh_poses and animate still give what a one-entry cast gives.
32 x 32 frames of the Cornell Box with the cast of tests/_cast_scene.py on it."""
import ctypes as C
import numpy as np
import pytest
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_animation_nodes_gpu import EVERY, bits
from _anim_model import F
from _cast_scene import Cast, cast_scene, FIRST_CHARACTER_INSTANCE, SPARE_MESH, TALL_BOX

pytestmark = pytest.mark.gpu
W = H = 32
CASTS = {"one mesh entry": ("tree257",), "one instance entry": ("crowd",), "five mixed entries": ("morph", "crowd", "chain2", "pair", "tree257")}
CHARACTERS = ("chain2", "tree257", "morph")


@pytest.fixture(scope="module")
def world(gpu):
    """(the cast, its host scene, the geometry of every mesh): made once, never changed."""
    fs, geo = cast_scene(gpu)
    return Cast(gpu), fs, geo


def _renderer(frt, fs, **kw):
    return frt.Renderer(fs, W, H, max_depth=2, **kw)


def _replica(r, rebuilt=False):
    return {w: r.read_scene(w).tobytes() for w in EVERY if not (rebuilt and w == "pair_nodes")}


def _same_replica(r, other, what, rebuilt=False):
    got, want = _replica(r, rebuilt), _replica(other, rebuilt)
    for x in got:
        assert got[x] == want[x], f"{what}: {x}"
    return got


def _same_bindings(cast, r, other, b, names, what):
    for name in names:
        if cast.is_instances(name):
            assert bits(r.read_rig_instances(b[name])) == bits(other.read_rig_instances(b[name])), f"{what}: matrices of {name}"
        else:
            got, want = r.read_rig_pose(b[name]), other.read_rig_pose(b[name])
            for g, w_, part in zip(got, want, ("palette", "weights")):
                assert (g is None) == (w_ is None) and (g is None or bits(g) == bits(w_)), f"{what}: {part} of {name}"


def _cast(r, b, rows, **kw):
    r.animate_cast([(b[name], clip, t) for name, clip, t in rows], **kw)


def _pair(frt, cast, fs, geo, names, **kw):
    """Two renderers over one scene with the same bindings under the same numbers."""
    r, other = _renderer(frt, fs, **kw), _renderer(frt, fs, **kw)
    b = cast.bind(r, geo, names)
    assert cast.bind(other, geo, names) == b
    return r, other, b


@pytest.mark.parametrize("which", list(CASTS))
def test_bit_equality_with_the_single_calls(gpu, world, which):
    frt = gpu
    cast, fs, geo = world
    names = CASTS[which]
    r, other, b = _pair(frt, cast, fs, geo, names, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); other.render(cam)
    start = _replica(r)
    steps = [[(name, "move", cast.times(name)[i]) for name in names] for i in range(3)] + [[(name, "rest", 0.0) for name in names]]
    for rows in steps:      # before the clip, on a key, between keys; then the second clip
        _cast(r, b, rows)
        cast.singles(other, b, rows if which != "five mixed entries" else rows[::-1])      # (singly, each kind in another order)
        what = f"{which}, {rows[0][1]} at {rows[0][2]}"
        got = _same_replica(r, other, what)
        _same_bindings(cast, r, other, b, names, what)
        assert got["tri_slots"] != start["tri_slots"]
    for name in names:      # and the buffers are the host's bits, as after the single calls
        if cast.is_instances(name):
            assert bits(r.read_rig_instances(b[name])) == bits(cast.rig[name].evaluate_nodes("rest", 0.0, cast.kw[name]["nodes"], cast.kw[name].get("root"), cast.kw[name].get("offsets")))
        else:
            want = cast.rig[name].evaluate("rest", 0.0)
            assert [None if x is None else bits(x) for x in r.read_rig_pose(b[name])] == [None if x is None else bits(x) for x in want]
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0) == (other.transform_rejects(), other.deform_rejects())
    for x in (r, other):
        x.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        r.render(cam); other.render(cam)
        assert r.read_accum().tobytes() == other.read_accum().tobytes(), f"{which}: frame {f}"


def test_a_character_on_a_moving_prop(gpu, world):
    """An instance entry moves the instances whose meshes a mesh entry of the same call poses: the pose's triangles are written under the matrix the
    first half left in the device table. Three frames in a row: from the second on the host's mirror of the matrices is stale on entry."""
    frt = gpu
    cast, fs, geo = world
    r, other = _renderer(frt, fs, flags=frt.FLAG_PIPELINE), _renderer(frt, fs, flags=frt.FLAG_PIPELINE)
    cast.bind_meshes(r, geo, ("chain2",)); cast.bind_meshes(other, geo, ("chain2",))
    carried = [FIRST_CHARACTER_INSTANCE, FIRST_CHARACTER_INSTANCE + 1]      # the instances of meshes 4 and 5
    off = np.tile(np.eye(4, dtype=F).reshape(16), (2, 1))
    off[:, [0, 5, 10]] = F(0.2)
    b = {}
    for x in (r, other):
        b = {"chain2": x.bind_rig(cast.rig["chain2"], cast.MESHES["chain2"]), "prop": x.bind_rig_instances(cast.rig["pair"], carried, [11, 5], offsets=off)}
    start = _replica(r)
    for i in range(3):
        t = cast.times("pair")[i]
        r.animate_cast([(b["chain2"], "move", cast.times("chain2")[i]), (b["prop"], "move", t)])
        other.animate_instances(b["prop"], "move", t)
        other.animate(b["chain2"], "move", cast.times("chain2")[i])
        got = _same_replica(r, other, f"frame {i}")
        assert got["tri_slots"] != start["tri_slots"] and got["instances_dev"] != start["instances_dev"]      # (against the scene as created)
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); other.render(cam)
    assert r.read_accum().tobytes() == other.read_accum().tobytes()


def test_the_halves_reject_independently(gpu, world):
    frt = gpu
    cast, fs, geo = world
    names = ("pair",) + CHARACTERS
    r, other, b = _pair(frt, cast, fs, geo, names)
    # a bound node scaled to zero: the instance half is rejected, the mesh half poses
    assert np.linalg.det(cast.rig["pair"].evaluate_nodes("vanish", 1.0, [3])[0].reshape(4, 4)[:3, :3]) == 0.0
    start = _replica(r)
    rows = [("tree257", "move", 0.5), ("pair", "vanish", 1.0), ("morph", "move", 0.5), ("chain2", "move", 0.5)]
    _cast(r, b, rows)
    cast.singles(other, b, rows)
    assert (r.transform_rejects(), r.deform_rejects()) == (1, 0) and other.transform_rejects() == 1
    got = _same_replica(r, other, "a rejected instance half")
    assert got["instances_dev"] == start["instances_dev"] and got["lights"] == start["lights"] and got["tri_slots"] != start["tri_slots"]
    # a palette that overflows in one of three characters: no character is posed, the instances move
    pal = cast.rig["chain2"].evaluate("burst", 1.0)[0]
    assert not np.isfinite(pal).all() and np.isfinite(cast.rig["chain2"].evaluate("burst", 0.0)[0]).all()
    start = got
    rows = [("morph", "move", 0.7), ("chain2", "burst", 1.0), ("pair", "move", 0.7), ("tree257", "move", 0.7)]
    _cast(r, b, rows)
    other.animate_instances(b["pair"], "move", 0.7)      # what the call applies: its instance half and nothing else
    assert (r.transform_rejects(), r.deform_rejects()) == (1, 1)
    got = _same_replica(r, other, "a rejected mesh half")
    assert got["instances_dev"] != start["instances_dev"] and got["attributes"] == start["attributes"]
    # the next clean cast applies normally
    rows = [(name, "move", cast.times(name)[2]) for name in names]
    _cast(r, b, rows)
    cast.singles(other, b, rows)
    assert (r.transform_rejects(), r.deform_rejects()) == (1, 1) and (other.transform_rejects(), other.deform_rejects()) == (1, 0)
    _same_replica(r, other, "a clean cast after the rejected ones")
    _same_bindings(cast, r, other, b, names, "a clean cast after the rejected ones")


def test_refusals(gpu, world):
    frt = gpu
    from frt._lib import check
    L = frt.lib()
    cast, fs, geo = world
    r = _renderer(frt, fs)
    b = cast.bind(r, geo, ("pair",) + CHARACTERS)
    again = r.bind_rig(cast.rig["chain2"], cast.MESHES["chain2"][1:])                    # a second binding on mesh 5
    shared = r.bind_rig_instances(cast.rig["pair"], [3, TALL_BOX], [0, 1])               # ... and one on instance 8
    unbound = r.bind_rig_instances(cast.rig["pair"], [2], [0])
    L.frt_renderer_unbind_rig(r._h, unbound)
    start, counters = _replica(r), (r.transform_rejects(), r.deform_rejects())

    def raw(rows, n=None, flags=0, null=False):
        table = (frt.CastEntry * max(len(rows), 1))(*[frt.CastEntry(*row) for row in rows])
        check(L.frt_renderer_animate_cast(r._h, len(rows) if n is None else n, None if null else table, flags))

    good = [(b["pair"], 0, 0.5, 0), (b["chain2"], 0, 0.5, 0)]
    refused = {
        "n == 0": lambda: raw([]),
        "n == 0 through the wrapper": lambda: r.animate_cast([]),
        "more than FRT_MAX_CAST_ENTRIES": lambda: raw(good * 2049),
        "null entries": lambda: raw(good, null=True),
        "reserved != 0": lambda: raw([good[0], (b["chain2"], 0, 0.5, 1)]),
        "unknown flag bits": lambda: raw(good, flags=4),
        "FRT_DEFORM_DEVICE is not the call's to take": lambda: raw(good, flags=frt.DEFORM_DEVICE),
        "an unknown binding": lambda: raw([good[0], (99, 0, 0.5, 0)]),
        "an unbound binding": lambda: raw([good[0], (unbound, 0, 0.5, 0)]),
        "a binding named twice": lambda: raw(good + [good[0]]),
        "a mesh two mesh entries would pose": lambda: raw(good + [(again, 0, 0.5, 0)]),
        "an instance two instance entries would move": lambda: raw(good + [(shared, 0, 0.5, 0)]),
        "a clip out of range": lambda: raw([good[0], (b["chain2"], cast.rig["chain2"].num_clips, 0.5, 0)]),
        "a clip name the rig does not have": lambda: r.animate_cast([(b["pair"], "burst", 0.5)]),
        "time is NaN": lambda: raw([good[0], (b["chain2"], 0, np.nan, 0)]),
        "time is +inf": lambda: raw([(b["pair"], 0, np.inf, 0), good[1]]),
        "time is -inf": lambda: raw([good[0], (b["chain2"], 0, -np.inf, 0)]),
    }
    for what, call in refused.items():
        with pytest.raises(frt.FrtError):
            call()
        assert _replica(r) == start and (r.transform_rejects(), r.deform_rejects()) == counters, what
    assert L.frt_renderer_animate_cast(None, 1, (frt.CastEntry * 1)(), 0) == -1
    # a mesh that no longer has the binding its rig implies
    mesh = cast.MESHES["tree257"][0]
    r.set_mesh_skin(mesh, None)
    with pytest.raises(frt.FrtError):
        raw([good[0], (b["tree257"], 0, 0.5, 0)])
    cast.bind_meshes(r, geo, ("tree257",))
    # inside an open frame
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    with pytest.raises(frt.FrtError, match="error -4"):
        raw(good)
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert _replica(r) == start and (r.transform_rejects(), r.deform_rejects()) == counters
    raw(good + [(b["tree257"], 0, 0.5, 0), (b["morph"], 1, 0.0, 0)], flags=frt.DEFORM_RECOMPUTE_NORMALS)      # and the good call applies
    assert _replica(r)["tri_slots"] != start["tri_slots"] and (r.transform_rejects(), r.deform_rejects()) == counters


def test_edits_between_casts(gpu, world):
    frt = gpu
    cast, fs, geo = world
    names = ("pair", "chain2", "spare")
    r, other, b = _pair(frt, cast, fs, geo, names)
    rows = [(name, "move", cast.times(name)[2]) for name in ("chain2", "pair")]
    _cast(r, b, rows)
    cast.singles(other, b, rows)
    for x in (r, other):
        x.remove_instances([2])      # unbound, below both instances of "pair": 8 becomes 7 and 7 becomes 6; the device copy of the ids is stale
    rows = [(name, "move", cast.times(name)[1]) for name in ("chain2", "pair")]
    _cast(r, b, rows)
    cast.singles(other, b, rows)
    _same_replica(r, other, "after remove_instances", rebuilt=True)
    _same_bindings(cast, r, other, b, ("chain2", "pair"), "after remove_instances")
    assert r.transform_rejects() == 0 and r.deform_rejects() == 0
    r.remove_meshes([SPARE_MESH])      # the binding "spare" names the mesh that left: it is unbound
    start = _replica(r, rebuilt=True)
    with pytest.raises(frt.FrtError):
        _cast(r, b, rows + [("spare", "move", 0.5)])
    assert _replica(r, rebuilt=True) == start
    _cast(r, b, rows)      # the others still hold


def test_the_shared_kernels_give_what_a_one_entry_cast_gives(gpu, world):
    """set_mesh_poses (host arrays: its own palette section), animate and a one-entry animate_cast on one character: the same replica."""
    frt = gpu
    cast, fs, geo = world
    rs = [_renderer(frt, fs) for _ in range(3)]
    for x in rs:
        cast.bind_meshes(x, geo, ("tree257",))
    b = [x.bind_rig(cast.rig["tree257"], cast.MESHES["tree257"]) for x in rs[1:]]
    start = _replica(rs[0])
    for t in cast.times("tree257"):
        rs[0].set_mesh_poses(cast.MESHES["tree257"], *cast.rig["tree257"].evaluate("move", t))
        rs[1].animate(b[0], "move", t)
        rs[2].animate_cast([(b[1], "move", t)])
        got = _same_replica(rs[0], rs[1], f"set_mesh_poses vs animate at {t}")
        _same_replica(rs[2], rs[1], f"animate_cast vs animate at {t}")
        assert got["tri_slots"] != start["tri_slots"]
    assert [x.deform_rejects() for x in rs] == [0, 0, 0]
