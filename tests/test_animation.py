"""frt_rig_evaluate, the host specification of the animation (include/frt.h; DESIGN.md section 11, "Animation"), against tests/_anim_model.py: the
identities the contract makes exact, bit for bit; the branches of the slerp; closeness to float64 on random rigs; acosf_ against np.arccos; what
frt_rig_create refuses; and SceneBuilder.animate = evaluate + set_mesh_poses."""
import numpy as np
import pytest
from test_mesh_deform import CUBE, SPHERE, EVERYTHING
from test_instance_update import cornell_meshes
from _skin_model import F, make_skin
from _morph_model import make_targets
from _anim_model import D, make_rig, make_channel, model_evaluate, sample_times, unit_quats

# Measured on the host (profiles/animation_f64.md): the largest max|f32 - f64| / max|f64| over a palette, 200 times per rig. The host form calls no
# libm and reproduces exactly; the test asserts twice the measured value, which covers another seed, not another platform.
F64_MEASURED = {"chain1": 4.81e-08, "chain2": 2.65e-07, "chain70": 1.90e-06, "fan65": 4.92e-07, "tree257": 4.46e-07, "tree1024": 5.67e-07}
ACOS_MAX_ULP = 1.25      # measured over the sweep of test_acos (profiles/animation_f64.md)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def one_node(path, interp, times, values, rest=None, num_targets=0):
    """A rig of one joint whose `path` has one channel."""
    desc = {"parents": [-1], "joint_nodes": [0], "num_targets": num_targets,
            "clips": [("c", [{"node": 0, "path": path, "interpolation": interp, "times": np.asarray(times, F), "values": np.asarray(values, F)}])]}
    desc.update(rest or {})
    return desc


@pytest.mark.parametrize("interp", ["STEP", "LINEAR", "CUBICSPLINE"])
def test_key_times_and_clamping_are_exact(frt, interp):
    rng = np.random.default_rng(3)
    for path in ("translation", "scale", "rotation"):
        ch = make_channel(rng, 0, path, interp, 6)
        desc = {"parents": [-1], "joint_nodes": [0], "clips": [("c", [ch])]}
        rig = frt.Rig(**desc)
        keys = ch["values"].reshape(6, 3, -1)[:, 1] if interp == "CUBICSPLINE" else ch["values"]
        cases = [(ch["times"][0] - 5.0, 0), (ch["times"][-1] + 5.0, 5), (np.nextafter(ch["times"][-1], F(9)), 5)] + [(ch["times"][k], k) for k in range(6)]
        for t, k in cases:
            want = dict(desc, clips=[("c", [dict(ch, interpolation="STEP", times=F([0]), values=keys[k:k + 1])])])
            assert bits(rig.evaluate(0, t)[0]).tolist() == bits(frt.Rig(**want).evaluate(0, 0.0)[0]).tolist(), (path, t, k)


def test_step_holds_and_a_clip_without_channels_gives_the_rest_pose(frt):
    desc = make_rig("tree257", seed=1)
    rig = frt.Rig(**desc)
    rest, rest_w = rig.evaluate("rest", 0.3)
    for t in (-1.0, 0.0, 2.5, 1e6):
        pal, w = rig.evaluate("rest", t)
        assert bits(pal).tolist() == bits(rest).tolist() and bits(w).tolist() == bits(desc["default_weights"]).tolist()
    assert bits(rest_w).tolist() == bits(desc["default_weights"]).tolist()
    mp, _ = model_evaluate(desc, 1, 0.0)
    assert np.abs(rest - mp).max() / np.abs(mp).max() < 4 * F64_MEASURED["tree257"]
    ch = make_channel(np.random.default_rng(5), 0, "translation", "STEP", 4)
    one = frt.Rig(parents=[-1], joint_nodes=[0], clips=[("c", [ch])])
    for k in range(3):
        for t in (ch["times"][k], (ch["times"][k] + ch["times"][k + 1]) / 2, np.nextafter(ch["times"][k + 1], F(-9))):
            assert bits(one.evaluate(0, t)[0][0, 12:15]).tolist() == bits(ch["values"][k]).tolist()


def test_rest_pose_with_exact_inverse_binds_is_the_identity_palette(frt):
    """Translations and scales by powers of two, half-turn and third-turn rotations as quaternions (their nine products are exact), quarter turns as
    matrix nodes: every product is exact, so global * inverse(global) is the identity to the bit."""
    rng = np.random.default_rng(11)
    n = 24
    par = np.array([-1] + [int(rng.integers(0, i)) for i in range(1, n)], np.int32)
    quats = np.array([[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, 0.5]], F)
    tr = (2.0 ** rng.integers(-2, 3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    ro = quats[rng.integers(0, len(quats), n)]
    sc = (2.0 ** rng.integers(-1, 2, (n, 3))).astype(F)
    quarter = np.array([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [4, -2, 0.5, 1]], F)      # a quarter turn about z and a translation; [c, r]
    mats = {5: quarter.reshape(16), 17: quarter.reshape(16)}
    desc = {"parents": par, "translations": tr, "rotations": ro, "scales": sc, "matrices": mats, "joint_nodes": rng.permutation(n).astype(np.uint32)}
    glob, _ = model_evaluate(dict(desc, clips=[("rest", [])]), 0, 0.0)
    inv = np.stack([np.linalg.inv(g.reshape(4, 4).T).T.reshape(16) for g in glob])
    assert np.array_equal(inv.astype(F).astype(D), inv)      # the inverses are float32 numbers
    rig = frt.Rig(**dict(desc, inverse_bind=inv.astype(F), clips=[("rest", [])]))
    pal, _ = rig.evaluate(0, 0.0)
    assert np.array_equal(pal, np.tile(np.eye(4, dtype=F).reshape(16), (n, 1)))


def test_slerp_branches(frt):
    q0 = unit_quats(np.random.default_rng(2), 1)[0]

    def turned(cos_half):      # q0 turned so that dot(q0, q) is about cos_half
        a = np.arccos(cos_half)
        x, y, z, w = q0.astype(D)
        dq = np.array([np.sin(a), 0.0, 0.0, np.cos(a)])      # q0 * dq
        X, Y, Z, W = dq
        return np.array([w * X + x * W + y * Z - z * Y, w * Y - x * Z + y * W + z * X, w * Z + x * Y - y * X + z * W, w * W - x * X - y * Y - z * Z]).astype(F)

    for name, q1 in (("the long way round", -turned(0.3)), ("just below 0.9995", turned(0.99949)), ("just above 0.9995", turned(0.99951)), ("wide", turned(0.2)),
                     ("equal", q0.copy()), ("opposite sign", -q0)):
        d = float(np.dot(q0.astype(D), q1.astype(D)))
        rig = frt.Rig(**one_node("rotation", "LINEAR", [0.0, 1.0], [q0, q1]))
        for u in (0.0, 1.0, 0.25, 0.5, float(np.nextafter(F(1), F(0)))):
            pal, _ = rig.evaluate(0, u)
            want, _ = model_evaluate(one_node("rotation", "LINEAR", [0.0, 1.0], [q0, q1]), 0, u)
            assert np.abs(pal - want).max() < 2e-6, (name, u, d)
            if u in (0.0, 1.0):      # the keys themselves, as stored
                key = frt.Rig(parents=[-1], joint_nodes=[0], rotations=[q0 if u == 0.0 else q1], clips=[("rest", [])]).evaluate(0, 0.0)[0]
                assert bits(pal).tolist() == bits(key).tolist(), (name, u)
        if d < 0.0:      # the short way: the rotation -q1 names is the one q1 names, and the path to it is the same
            flipped = frt.Rig(**one_node("rotation", "LINEAR", [0.0, 1.0], [q0, -q1]))
            assert np.abs(rig.evaluate(0, 0.5)[0] - flipped.evaluate(0, 0.5)[0]).max() < 2e-6, name


def test_slerp_switches_to_the_mix_exactly_above_0_9995(frt):
    """Pairs whose float32 dot product (in the contract's association) lies a few ulp either side of float32(0.9995). At that angle the two formulas
    differ by about 1e-8, less than any tolerance against float64 could see, so each side is held to the float32 bits of its own formula, restated here
    in numpy float32 scalars: the mix, and the spherical form with the library's acos (frt_acosf) and the sine polynomial of frt_math.hpp's sincosf_
    (angles below pi/4: no reduction). That the two restatements differ at some u is asserted too: otherwise the test could not tell the branches apart."""
    thr = F(0.9995)

    def dot(a, b):
        return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])) + F(a[3] * b[3])

    def mix(q0, q1, u):      # the contract's d > 0.9995 branch in float32
        u = F(u)
        q = F(q0 * F(F(1) - u)) + F(q1 * u)
        dd = dot(q, q)
        return F(q * F(F(1) / np.sqrt(dd)))

    def sin_small(x):      # sincosf_'s sine for |x| < pi/4 (q = 0: r = x)
        z = F(x * x)
        return F(F(F(F(F(F(F(-1.9515295891e-4) * z) + F(8.3321608736e-3)) * z) - F(1.6666654611e-1)) * z) * x) + x

    def acos32(d):
        x, out = F([d]), F([0])
        frt.lib().frt_acosf(1, x.ctypes.data, out.ctypes.data)
        return out[0]

    def spherical(q0, q1, u):      # the contract's other branch in float32
        u, th = F(u), acos32(dot(q0, q1))
        inv = F(F(1) / sin_small(th))
        w0, w1 = F(sin_small(F(F(F(1) - u) * th)) * inv), F(sin_small(F(u * th)) * inv)
        return F(F(q0 * w0) + F(q1 * w1))

    q0 = F([0.0, 0.0, 0.0, 1.0])
    sides = {"above": [], "below": []}
    for k in range(-4, 5):
        wk = thr
        for _ in range(abs(k)):
            wk = np.nextafter(wk, F(2) if k > 0 else F(0))
        q1 = F([np.sqrt(np.float64(1) - np.float64(wk) ** 2), 0.0, 0.0, wk])
        assert dot(q0, q1) == wk
        sides["above" if wk > thr else "below"].append(q1)
    assert len(sides["above"]) == 4 and len(sides["below"]) == 5      # d == 0.9995f itself is not above
    rest = lambda q: frt.Rig(parents=[-1], joint_nodes=[0], rotations=[q], clips=[("rest", [])]).evaluate(0, 0.0)[0]      # noqa: E731
    differ = 0
    for side, qs in sides.items():
        for q1 in qs:
            rig = frt.Rig(**one_node("rotation", "LINEAR", [0.0, 1.0], [q0, q1]))
            for u in (0.125, 0.25, 0.5, 0.7, 0.9):
                got, mixed, round_way = (bits(x).tolist() for x in (rig.evaluate(0, u)[0], rest(mix(q0, q1, u)), rest(spherical(q0, q1, u))))
                differ += mixed != round_way
                assert got == (mixed if side == "above" else round_way), (side, q1[3], u)
    assert differ >= 20      # of 45 cases


@pytest.mark.parametrize("shape", list(F64_MEASURED))
def test_random_rigs_are_close_to_float64(frt, shape):
    desc = make_rig(shape)
    rig = frt.Rig(**desc)
    assert rig.num_nodes == len(desc["parents"]) and rig.num_joints == rig.num_nodes
    worst = worst_w = 0.0
    for t in sample_times(desc, 200):
        pal, w = rig.evaluate(0, t)
        mp, mw = model_evaluate(desc, 0, t)
        worst = max(worst, float(np.abs(pal - mp).max() / np.abs(mp).max()))
        worst_w = max(worst_w, float(np.abs(w - mw).max()))
    print(f"{shape}: max |f32 - f64| / max |f64| = {worst:.3e}; weights: {worst_w:.3e}")
    assert worst <= 2 * F64_MEASURED[shape]
    assert worst_w <= 8 * 2.0 ** -24      # a few roundings of numbers of size one (the cubic's four products and three sums)


def test_acos(frt):
    x = np.linspace(-1, 1, 2000001).astype(F)
    near_one = np.arange(F(0.99).view(np.uint32), F(1).view(np.uint32) + 1, dtype=np.uint32).view(F)      # every float32 in [0.99, 1]
    x = np.concatenate([x, near_one, -near_one, F([0.5, -0.5, 0.0, 1.0, -1.0])])
    got = np.zeros_like(x)
    frt.lib().frt_acosf(x.size, x.ctypes.data, got.ctypes.data)
    want = np.arccos(x.astype(D))
    ulp = np.spacing(np.maximum(want.astype(F), F(1e-30))).astype(D)
    err = np.abs(got.astype(D) - want) / ulp
    print(f"acosf_: max error {err.max():.3f} ulp at x = {x[err.argmax()]!r}")
    assert err.max() <= ACOS_MAX_ULP
    assert got[-2] == 0.0 and got[-1] == F(np.pi)
    edge = F([1.5, -1.5, np.nan])
    out = np.zeros_like(edge)
    frt.lib().frt_acosf(3, edge.ctypes.data, out.ctypes.data)
    assert out[0] == 0.0 and out[1] == F(np.pi) and np.isnan(out[2])


def test_refusals(frt):
    good = make_rig("chain2", keys=(5,))
    frt.Rig(**good)
    ch = good["clips"][0][1][0]

    def with_channel(**kw):
        return dict(good, clips=[("c", [dict(ch, **kw)])])

    k = len(ch["times"])
    bad = [dict(good, parents=[0, -1]), dict(good, parents=[-1, 1]), dict(good, parents=[-2, 0]),            # a cycle, a later parent
           dict(good, joint_nodes=[0, 2]),                                                                    # a joint that is not a node
           dict(good, joint_nodes=[], inverse_bind=None, num_targets=0, default_weights=None, clips=[]),      # neither joints nor targets
           dict(good, num_targets=5000, default_weights=None, clips=[]),
           dict(good, translations=F([[0, 0, 0], [np.inf, 0, 0]])),
           with_channel(node=7), with_channel(times=ch["times"][::-1].copy()),
           with_channel(times=np.full(k, np.nan, F)), with_channel(values=np.full_like(ch["values"], np.nan)),
           dict(good, clips=[("c", [ch, ch])]),                                                               # the same node and path twice
           dict(good, matrices={0: np.eye(4, dtype=F).reshape(16)}, clips=[("c", [dict(ch, node=0)])])]       # a channel on a matrix node
    for b in bad:
        with pytest.raises(frt.FrtError):
            frt.Rig(**b)
    with pytest.raises(frt.FrtError):      # an output count that does not match the input count
        frt.Rig(**with_channel(values=ch["values"][:-1]))
    two = frt.Rig(**make_rig("chain2", keys=(2,)))
    dup = make_rig("chain2", keys=(2,))
    dup["clips"][0][1][0]["times"] = F([0.5, 0.5])
    with pytest.raises(frt.FrtError, match="strictly increasing"):
        frt.Rig(**dup)
    for clip, t in ((2, 0.0), (0, np.nan), (0, np.inf), (0, -np.inf), (0, 1e39)):
        with pytest.raises(frt.FrtError):
            two.evaluate(clip, t)
    with pytest.raises(frt.FrtError, match="no clip named"):
        two.evaluate("walk", 0.0)
    L = frt.lib()
    assert not L.frt_rig_create(None) and b"null" in L.frt_last_error()
    assert L.frt_rig_evaluate(None, 0, 0.0, None, None) == -1 and L.frt_rig_evaluate(two._h, 0, 0.0, None, None) == -1


def test_scene_animate_is_evaluate_then_set_mesh_poses(frt):
    meshes = cornell_meshes(frt)
    ids = [CUBE, SPHERE]
    desc = make_rig("tree257", seed=2, joints="subset", num_targets=4)
    rig = frt.Rig(**desc)
    a, b = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    before = a.get("tri_slots").tobytes()
    for s in (a, b):
        for m in ids:
            n = len(meshes[m].positions)
            s.set_mesh_morph_targets(m, 0.1 * make_targets(n, rig.num_targets, seed=m))
            s.set_mesh_skin(m, *make_skin(n, rig.num_joints, seed=m), num_joints=rig.num_joints)
    for t in sample_times(desc, 3):
        a.animate(rig, ids, "move", t)
        b.set_mesh_poses(ids, *rig.evaluate("move", t))
        for w in EVERYTHING:
            assert a.get(w).tobytes() == b.get(w).tobytes(), w
    assert a.get("tri_slots").tobytes() != before
