"""Node animation on the device (include/frt.h: frt_renderer_bind_rig_instances, _animate_instances, _read_rig_instances; DESIGN.md section 11, "Node
animation"): the kernel's matrices are frt_rig_evaluate_nodes', bit for bit, on the rig shapes and instance counts at which it could go wrong; after
animate_instances the replica equals that of a renderer given the host-evaluated matrices through set_instance_transforms, frames included, and a
registered light follows its instance; a node scaled to zero rejects the call on the device; a binding follows remove_instances; what cannot be
bound or animated is refused with nothing enqueued; a MultiRenderer's strips follow. 32 x 32 frames of the Cornell Box (9 instances, 8 the tall box)."""
import ctypes as C
import numpy as np
import pytest
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import PLANE, SPHERE
from test_instance_update import cornell_meshes
from _skin_model import make_skin
from _anim_model import F, make_rig, sample_times

pytestmark = pytest.mark.gpu
W = H = 32
EVERY = ("tri_slots", "pair_nodes", "quad_nodes", "shade_tris", "attributes", "normals", "instances_dev", "lights")
TALL_BOX = 8
# the smallest rigs at which the kernel can go wrong
SHAPES = {"one node": "chain1", "more levels than a wave has lanes": "chain70", "a level past the wave": "fan65", "past the workgroup's stride": "tree257",
          "the LDS limit": "tree1024"}
COUNTS = (1, 9, 300)      # one lane, the Cornell Box, past the 256-lane stride of the kernel's last phase


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32).tolist()


def _replica(r, rebuilt=False):
    """rebuilt: after a device rebuild (an instance or a light was added or removed) the pair tree no longer describes the replica and cannot be read."""
    return {w: r.read_scene(w).tobytes() for w in EVERY if not (rebuilt and w == "pair_nodes")}


def _renderer(frt, fs=None, **kw):
    return frt.Renderer(fs or frt.scenes.create_cornell_box(), W, H, max_depth=2, **kw)


def near_identity(rng, n, spread=0.1):
    m = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (spread * rng.standard_normal((n, 9))).astype(F)
    m[:, 12:15] = (spread * rng.standard_normal((n, 3))).astype(F)
    return m


def small_rig(frt, extra_clips=(), seed=4):
    """(description, rig): 12 nodes without joints, moved towards the origin so that what hangs on them stays about the box."""
    desc = make_rig("tree12", seed=seed, joints="none", num_targets=0, keys=(2, 5))
    desc["translations"] = F(0.2) * desc["translations"]
    for ch in desc["clips"][0][1]:
        if ch["path"] == "translation":
            ch["values"] = F(0.3) * ch["values"]
    desc["clips"] = desc["clips"] + list(extra_clips)
    return desc, frt.Rig(**desc, nodes_only=True)


def three_times(desc):
    t = sample_times(desc, 9)      # before the clip, a key time, between keys
    return F([t[0], t[4], t[8]])


@pytest.fixture(scope="module")
def crowd(gpu):
    """One renderer for the bit tests: the Cornell Box and 291 small planes, 300 instances."""
    frt = gpu
    r = _renderer(frt)
    rng = np.random.default_rng(11)
    mats = np.tile(np.eye(4, dtype=F).reshape(16), (291, 1))
    mats[:, [0, 5, 10]] = F(0.02)
    mats[:, 12:15] = rng.uniform(-0.8, 0.8, (291, 3)).astype(F)
    assert r.add_instances([PLANE] * 291, [0] * 291, mats) == 9
    return r


@pytest.mark.parametrize("which", list(SHAPES))
def test_matrices_have_the_host_bits(gpu, crowd, which):
    frt, r = gpu, crowd
    shape = SHAPES[which]
    rng = np.random.default_rng(len(shape))
    root = near_identity(rng, 1)[0]
    rejects = r.transform_rejects()
    for joints in ("none", "all"):
        desc = make_rig(shape, joints=joints, num_targets=0, keys=(1, 2, 33))
        rig = frt.Rig(**desc, nodes_only=joints == "none")
        for n in COUNTS:
            ids = [TALL_BOX] if n == 1 else rng.permutation(n)
            nodes = rng.integers(0, rig.num_nodes, n)
            for kw in ({}, {"root": root, "offsets": near_identity(rng, n)}):
                b = r.bind_rig_instances(rig, ids, nodes, **kw)
                assert not r.read_rig_instances(b).any()      # zeros before the first animate_instances
                for clip, times in ((0, three_times(desc)), (1, F([0.0]))):
                    for t in times:
                        r.animate_instances(b, clip, t)
                        assert bits(r.read_rig_instances(b)) == bits(rig.evaluate_nodes(clip, t, nodes, **kw)), f"{which}, joints {joints}, n {n}, {sorted(kw)}: clip {clip} at {t}"
                r.unbind_rig(b)
                with pytest.raises(frt.FrtError):
                    r.animate_instances(b, 0, 0.0)
    assert r.transform_rejects() == rejects


def test_replica_and_frames_equal_the_host_route(gpu):
    frt = gpu
    desc, rig = small_rig(frt)
    fs = frt.scenes.create_cornell_box()
    r, other = _renderer(frt, fs, flags=frt.FLAG_PIPELINE), _renderer(frt, fs, flags=frt.FLAG_PIPELINE)
    lamp = np.eye(4, dtype=F)
    lamp[[0, 1, 2], [0, 1, 2]] = F(0.1)
    for x in (r, other):
        assert x.register_sphere_light(SPHERE, lamp, (1.0, 0.9, 0.8), 20.0) == fs.num_lights      # instance 9 carries it
    nl = fs.num_lights + 1
    cam = frt.CameraController().build_uniform(W / H, 0, nl)
    r.render(cam); other.render(cam)
    start = _replica(r, rebuilt=True)
    ids, nodes = [TALL_BOX, 9, 7], [11, 5, 0]
    root = np.eye(4, dtype=F)
    root[3, :3] = (0.1, -0.2, 0.1)
    off = near_identity(np.random.default_rng(2), 3, 0.02)
    off[:, [0, 5, 10]] *= F([[0.3], [0.1], [0.3]])
    b = r.bind_rig_instances(rig, ids, nodes, root=root, offsets=off)
    for clip, t in (("move", three_times(desc)[0]), ("move", three_times(desc)[2]), ("rest", 0.0)):
        r.animate_instances(b, clip, t)
        mats = rig.evaluate_nodes(clip, t, nodes, root, off)
        assert bits(r.read_rig_instances(b)) == bits(mats)
        other.set_instance_transforms(ids, mats)
        got, want = _replica(r, rebuilt=True), _replica(other, rebuilt=True)
        for x in got:
            assert got[x] == want[x], f"animate_instances vs set_instance_transforms, {clip} at {t}: {x}"
    assert got["tri_slots"] != start["tri_slots"] and got["lights"] != start["lights"]      # the light record went with instance 9
    assert r.transform_rejects() == 0
    for x in (r, other):
        x.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, nl)
        r.render(cam); other.render(cam)
        assert r.read_accum().tobytes() == other.read_accum().tobytes(), f"frame {f}"


def test_a_node_scaled_to_zero_rejects_the_call_on_the_device(gpu):
    frt = gpu
    vanish = {"node": 3, "path": "scale", "interpolation": "LINEAR", "times": F([0.0, 1.0]), "values": F([[1, 1, 1], [0, 0, 0]])}
    desc, rig = small_rig(frt, extra_clips=[("vanish", [vanish])])
    fs = frt.scenes.create_cornell_box()
    r, untouched = _renderer(frt, fs), _renderer(frt, fs)
    ids, nodes = [TALL_BOX, 7], [3, 0]
    off = near_identity(np.random.default_rng(2), 2, 0.0)
    off[:, [0, 5, 10]] = F(0.3)
    assert np.linalg.det(rig.evaluate_nodes("vanish", 1.0, nodes)[0].reshape(4, 4)[:3, :3]) == 0.0
    b = r.bind_rig_instances(rig, ids, nodes, offsets=off)
    start = _replica(r)
    r.animate_instances(b, "vanish", 1.0)
    assert r.transform_rejects() == 1
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], f"a rejected animate_instances changed {x}"
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); untouched.render(cam)
    assert r.read_accum().tobytes() == untouched.read_accum().tobytes()
    r.animate_instances(b, "vanish", 0.5)      # and at another time the call applies
    untouched.set_instance_transforms(ids, rig.evaluate_nodes("vanish", 0.5, nodes, offsets=off))
    now, want = _replica(r), _replica(untouched)
    assert r.transform_rejects() == 1 and now["tri_slots"] != start["tri_slots"]
    for x in EVERY:
        assert now[x] == want[x], x


def test_a_binding_follows_remove_instances_and_numbers_are_reused(gpu):
    frt = gpu
    desc, rig = small_rig(frt)
    fs = frt.scenes.create_cornell_box()
    r, fresh = _renderer(frt, fs), _renderer(frt, fs)
    off = near_identity(np.random.default_rng(2), 1, 0.0)
    off[:, [0, 5, 10]] = F(0.3)
    b, lost = r.bind_rig_instances(rig, [TALL_BOX], [7], offsets=off), r.bind_rig_instances(rig, [6], [2])
    assert (b, lost) == (0, 1)
    for x in (r, fresh):
        x.remove_instances([2])      # unbound, below both: 8 becomes 7 and 6 becomes 5
    t = three_times(desc)[2]
    r.animate_instances(b, "move", t)
    fresh.set_instance_transforms([TALL_BOX - 1], rig.evaluate_nodes("move", t, [7], offsets=off))
    got, want = _replica(r, rebuilt=True), _replica(fresh, rebuilt=True)
    for x in got:
        assert got[x] == want[x], x
    r.remove_instances([5])      # the instance of the second binding: it is unbound
    with pytest.raises(frt.FrtError, match="unknown rig binding"):
        r.animate_instances(lost, "move", t)
    r.animate_instances(b, "move", t)      # 7 became 6; the first binding still holds
    assert r.bind_rig_instances(rig, [0], [0]) == lost      # the freed number is given out again
    r.unbind_rig(b)
    n = len(cornell_meshes(frt)[SPHERE].positions)
    skinned = frt.Rig(**make_rig("tree12", num_targets=0))
    r.set_mesh_skin(SPHERE, *make_skin(n, skinned.num_joints), num_joints=skinned.num_joints)
    assert r.bind_rig(skinned, [SPHERE]) == b      # ... by bind_rig too: one list of numbers
    with pytest.raises(frt.FrtError, match="binds meshes"):
        r.animate_instances(b, 0, 0.0)
    with pytest.raises(frt.FrtError, match="binds instances"):
        r.animate(lost, 0, 0.0)
    with pytest.raises(frt.FrtError):
        r.read_rig_instances(b)
    assert r.transform_rejects() == 0


def test_refusals(gpu):
    frt = gpu
    L = frt.lib()
    desc, rig = small_rig(frt)
    fs = frt.scenes.create_cornell_box()
    r = _renderer(frt, fs)
    start = _replica(r)
    eye = np.eye(4, dtype=F).reshape(16)
    too_many = frt.Rig(**make_rig("chain1025", joints="none", num_targets=0), nodes_only=True)
    assert too_many.num_nodes == frt.MAX_RIG_NODES + 1
    with pytest.raises(frt.FrtError, match="error -1"):      # a nodes-only rig poses no mesh
        r.bind_rig(rig, [SPHERE])
    many = np.arange(65537)
    for bad_rig, ids, nodes in ((too_many, [8], [0]), (rig, [], []), (rig, many, many * 0), (rig, [9], [0]), (rig, [8, 3, 8], [0, 1, 2]), (rig, [8], [12])):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.bind_rig_instances(bad_rig, ids, nodes)
    for bad in (np.nan, np.inf, -np.inf):
        m = eye.copy()
        m[13] = bad
        with pytest.raises(frt.FrtError, match="root entry is not finite"):
            r.bind_rig_instances(rig, [8], [0], root=m)
        with pytest.raises(frt.FrtError, match="offsets entry is not finite"):
            r.bind_rig_instances(rig, [8, 7], [0, 1], offsets=[eye, m])
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    b = r.bind_rig_instances(rig, [8], [0])
    assert b == 0      # the refused calls took no number
    call = L.frt_renderer_animate_instances
    assert call(r._h, b + 1, 0, 0.0) == -1                                  # an unknown binding
    assert call(r._h, b, rig.num_clips, 0.0) == -1                          # clip out of range
    for t in (np.nan, np.inf, -np.inf):
        assert call(r._h, b, 0, t) == -1                                    # a time that is not finite
    assert call(None, b, 0, 0.0) == -1
    assert L.frt_renderer_animate(r._h, b, 0, 0.0, 0) == -1                 # animate takes mesh bindings
    assert L.frt_renderer_read_rig_instances(r._h, b + 1, None) == -1 and L.frt_renderer_read_rig_instances(r._h, b, None) == -1
    r.render_phases(cam, frt.PHASE_GBUFFER)
    assert call(r._h, b, 0, 0.0) == -4                                      # inside an open frame
    ids, nodes, out = np.array([7], np.uint32), np.zeros(1, np.uint32), C.byref(C.c_uint32())
    assert L.frt_renderer_bind_rig_instances(r._h, rig._h, 1, ids.ctypes.data, nodes.ctypes.data, None, None, out) == -4
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert L.frt_renderer_bind_rig_instances(r._h, None, 1, ids.ctypes.data, nodes.ctypes.data, None, None, out) == -1
    assert L.frt_renderer_bind_rig_instances(r._h, rig._h, 1, None, nodes.ctypes.data, None, None, out) == -1
    assert L.frt_renderer_bind_rig_instances(r._h, rig._h, 1, ids.ctypes.data, nodes.ctypes.data, None, None, None) == -1
    assert r.transform_rejects() == 0
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], x
    r.animate_instances(b, "move", 0.5)                                     # and the good call applies
    assert r.transform_rejects() == 0 and r.read_scene("tri_slots").tobytes() != start["tri_slots"]


def test_multi_renderer(gpu):
    """Two strips on one device: the frame equals that of a single renderer animated on the device."""
    frt = gpu
    desc, rig = small_rig(frt)
    fs = frt.scenes.create_cornell_box()
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0], max_depth=2), frt.Renderer(fs, 64, 48, max_depth=2, flags=frt.FLAG_PIPELINE)
    ids, nodes = [TALL_BOX, 7], [11, 0]
    off = near_identity(np.random.default_rng(2), 2, 0.0)
    off[:, [0, 5, 10]] = F(0.3)
    b = one.bind_rig_instances(rig, ids, nodes, offsets=off)
    for t in three_times(desc)[1:]:
        multi.animate_instances(rig, ids, nodes, "move", t, offsets=off)
        one.animate_instances(b, "move", t)
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), t
