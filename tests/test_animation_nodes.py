"""Node animation on the host (include/frt.h: frt_rig_create_ex, frt_rig_evaluate_nodes; DESIGN.md section 11, "Node animation"): evaluate_nodes is tied
to the palette of frt_rig_evaluate bit for bit, held to the float64 model with a root, refuses what the header says it refuses, and
SceneBuilder.animate_instances is evaluate_nodes followed by set_instance_transforms."""
import ctypes as C
import numpy as np
import pytest
from test_mesh_deform import EVERYTHING
from _anim_model import F, D, make_rig, model_evaluate, sample_times, mat_mul

SHAPES = ("chain1", "chain2", "chain70", "fan65", "tree257", "tree1024")
# Measured on the host (profiles/animation_nodes_f64.md): the largest max|f32 - f64| / max|f64| over (root * global) * offset of every joint node, 200
# times per rig. The host form calls no libm and reproduces exactly; the test asserts twice the measured value, which covers another seed, not another
# platform (the margin of tests/test_animation.py).
F64_MEASURED = {"chain1": 7.54e-08, "chain2": 2.52e-07, "chain70": 1.53e-06, "fan65": 3.95e-07, "tree257": 4.97e-07, "tree1024": 5.36e-07}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32).tolist()


def a_root(seed=5):
    """A column-major affine matrix near a rotation, with a translation."""
    rng = np.random.default_rng(seed)
    m = np.eye(4, dtype=F)
    m[:3, :3] += (0.2 * rng.standard_normal((3, 3))).astype(F)
    m[3, :3] = (0.5 * rng.standard_normal(3)).astype(F)
    return m.reshape(16)


def three_times(desc):
    """Before the clip, a key time, between keys."""
    t = sample_times(desc, 9)
    return F([t[0], t[4], t[8]])


@pytest.mark.parametrize("shape", SHAPES)
def test_evaluate_nodes_with_inverse_binds_is_the_palette(frt, shape):
    desc = make_rig(shape)
    rig = frt.Rig(**desc)
    joints, ib = desc["joint_nodes"], desc["inverse_bind"]
    assert len(joints) == rig.num_nodes
    for clip, times in ((0, three_times(desc)), (1, F([0.0]))):
        for t in times:
            assert bits(rig.evaluate_nodes(clip, t, joints, offsets=ib)) == bits(rig.evaluate(clip, t)[0]), f"{shape}: clip {clip} at {t}"


@pytest.mark.parametrize("shape", SHAPES)
def test_root_and_offsets_are_close_to_float64(frt, shape):
    desc = make_rig(shape)
    rig = frt.Rig(**desc)
    joints, ib, root = desc["joint_nodes"], desc["inverse_bind"], a_root()
    root64 = root.astype(D).reshape(4, 4)
    worst = 0.0
    for t in sample_times(desc, 200):
        got = rig.evaluate_nodes(0, t, joints, root=root, offsets=ib)
        pal = model_evaluate(desc, 0, t)[0]
        want = np.stack([mat_mul(root64, p.reshape(4, 4)).reshape(16) for p in pal])
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"{shape}: max |f32 - f64| / max |f64| = {worst:.3e}")
    assert worst <= 2 * F64_MEASURED[shape]


def test_none_is_no_multiplication(frt):
    """root=None and offsets=None give the bits of the forms without them; an identity would not (it turns -0 into +0)."""
    desc = make_rig("tree257", seed=1)
    rig = frt.Rig(**desc)
    nodes, ib, root = desc["joint_nodes"][:40], desc["inverse_bind"][:40], a_root()
    eye = np.eye(4, dtype=F).reshape(16)
    for t in three_times(desc):
        plain = rig.evaluate_nodes(0, t, nodes)
        assert bits(rig.evaluate_nodes(0, t, nodes, root=None, offsets=None)) == bits(plain)
        assert bits(rig.evaluate_nodes(0, t, nodes, root=None, offsets=ib)) == bits(rig.evaluate_nodes(0, t, nodes, offsets=ib))
        assert bits(rig.evaluate_nodes(0, t, nodes, root=root, offsets=None)) == bits(rig.evaluate_nodes(0, t, nodes, root=root))
    # a global with a negative zero: a translation of -0 stays -0 without root and offsets
    rig = frt.Rig(parents=[-1], translations=F([[-0.0, 1.0, 2.0]]), nodes_only=True, clips=[("rest", [])])
    m = rig.evaluate_nodes(0, 0.0, [0])
    assert np.signbit(m[0, 12]) and not np.signbit(rig.evaluate_nodes(0, 0.0, [0], root=eye)[0, 12])


def test_nodes_are_the_callers_numbers(frt):
    """frt_rig_create stores the nodes by depth; evaluate_nodes still takes the numbers of the description."""
    par = np.array([-1, 0, 1, 0, -1, 4], np.int32)      # depths 0 1 2 1 0 1: stored order 0 4 1 3 5 2
    tr = np.arange(18, dtype=F).reshape(6, 3)
    rig = frt.Rig(parents=par, translations=tr, nodes_only=True, clips=[("rest", [])])
    got = rig.evaluate_nodes("rest", 0.0, [0, 1, 2, 3, 4, 5])[:, 12:15]
    want = np.stack([tr[0], tr[0] + tr[1], tr[0] + tr[1] + tr[2], tr[0] + tr[3], tr[4], tr[4] + tr[5]])
    assert np.array_equal(got, want)


def test_a_nodes_only_rig(frt):
    desc = make_rig("tree12", joints="none", num_targets=0)
    with pytest.raises(frt.FrtError, match="joints, morph targets or both"):
        frt.Rig(**desc)
    rig = frt.Rig(**desc, nodes_only=True)
    assert (rig.num_nodes, rig.num_joints, rig.num_targets, rig.num_clips) == (12, 0, 0, 2)
    assert rig.evaluate("move", 0.5) == (None, None)
    with_joints = frt.Rig(**dict(desc, joint_nodes=np.arange(12)[::-1]), nodes_only=True)      # the flag only lifts the one check
    assert with_joints.num_joints == 12
    nodes = list(range(12))
    assert bits(rig.evaluate_nodes("move", 0.5, nodes)) == bits(with_joints.evaluate_nodes("move", 0.5, nodes))
    s = frt.scenes.create_cornell_box()
    with pytest.raises(frt.FrtError):      # it poses no mesh
        s.animate(rig, [0], "move", 0.5)
    L = frt.lib()
    assert not L.frt_rig_create_ex(None, 1) and not L.frt_rig_create_ex(None, 2)
    assert b"unknown flag" in L.frt_last_error()


def test_refusals(frt):
    desc = make_rig("chain2", keys=(2,))
    rig = frt.Rig(**desc)
    root, off = a_root(), np.tile(np.eye(4, dtype=F).reshape(16), (2, 1))
    rig.evaluate_nodes(0, 0.5, [0, 1], root, off)
    for clip, t in ((2, 0.0), (0, np.nan), (0, np.inf), (0, -np.inf), (0, 1e39)):      # clip out of range, a time that is not finite
        with pytest.raises(frt.FrtError, match="error -1"):
            rig.evaluate_nodes(clip, t, [0])
    for nodes in ([2], [0, 1, 0xFFFFFFFF], []):      # a node that is not a node, n == 0
        with pytest.raises(frt.FrtError, match="error -1"):
            rig.evaluate_nodes(0, 0.5, nodes)
    for bad in (np.nan, np.inf, -np.inf):
        r, o = root.copy(), off.copy()
        r[7], o[1, 3] = bad, bad
        with pytest.raises(frt.FrtError, match="root entry is not finite"):
            rig.evaluate_nodes(0, 0.5, [0, 1], root=r)
        with pytest.raises(frt.FrtError, match="offsets entry is not finite"):
            rig.evaluate_nodes(0, 0.5, [0, 1], offsets=o)
    with pytest.raises(frt.FrtError):      # offsets not shaped [n, 16]
        rig.evaluate_nodes(0, 0.5, [0], offsets=off)
    no_clips = frt.Rig(parents=[-1], nodes_only=True)      # a rig without clips has no clip 0 (include/frt.h says so)
    with pytest.raises(frt.FrtError, match="out of range"):
        no_clips.evaluate_nodes(0, 0.0, [0])
    L = frt.lib()
    nodes, out = np.zeros(1, np.uint32), np.zeros(16, F)
    call = L.frt_rig_evaluate_nodes
    assert call(rig._h, 0, 0.5, 1, nodes.ctypes.data, None, None, out.ctypes.data) == 0
    assert call(rig._h, 0, 0.5, 1, nodes.ctypes.data, None, None, None) == -1      # a null output
    assert call(rig._h, 0, 0.5, 1, None, None, None, out.ctypes.data) == -1
    assert call(rig._h, 0, 0.5, 0, nodes.ctypes.data, None, None, out.ctypes.data) == -1
    assert call(None, 0, 0.5, 1, nodes.ctypes.data, None, None, out.ctypes.data) == -1


def test_scene_animate_instances_is_evaluate_nodes_then_set_instance_transforms(frt):
    desc = make_rig("tree12", seed=4, joints="none", num_targets=0)
    rig = frt.Rig(**desc, nodes_only=True)
    a, b = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    before = a.get("tri_slots").tobytes()
    ids, nodes = [8, 7, 2], [11, 3, 0]
    root = (np.eye(4, dtype=F) * F([0.3, 0.3, 0.3, 1.0])).reshape(16)      # the rig's nodes wander about the origin: keep the boxes small
    off = np.tile(np.eye(4, dtype=F).reshape(16), (3, 1))
    off[:, 12:15] = F([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, -0.1]])
    for t in three_times(desc):
        a.animate_instances(rig, ids, nodes, "move", t, root=root, offsets=off)
        b.set_instance_transforms(ids, rig.evaluate_nodes("move", t, nodes, root, off))
        for w in EVERYTHING:
            assert a.get(w).tobytes() == b.get(w).tobytes(), w
    assert a.get("tri_slots").tobytes() != before
