"""frt_rig_evaluate_layers_ik and frt_rig_evaluate_nodes_layers_ik, the host specification of inverse kinematics on a rig (include/frt.h; DESIGN.md
section 11, "Inverse kinematics"), against tests/_ik_model.py: what the contract makes exact, bit for bit; what a goal is for (the tip on its target,
bone lengths kept, the pole's side, the aimed axis); closeness to float64 for 1, 2 and 16 goals of both kinds over layered poses with every threshold
decision of the model kept clear of its threshold; the degenerate branches, decision by decision; every refusal with the outputs untouched; the new
symbols; and the host form, stand-alone, under a sanitiser."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from _skin_model import F
from _blend_model import make_blend_rig
from _layers_model import L, to_layers, random_masks, random_stacks, threshold_branch_gap
from _ik_model import TB, AIM, D, to_goals, model_evaluate_layers_ik, model_globals_ik, layered_globals, random_goals, random_targets, subtree_flags, unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("chain3", "chain70", "tree257", "tree1024")      # chain3: the smallest two-bone limb (the tip's subtree is the tip alone)
GOAL_COUNTS = (1, 2, 16)
# Measured on the host (profiles/animation_ik_f64.md): per shape the largest max|f32 - f64| / max|f64| over a palette and a matrix set over the
# chained cases of test_goals_are_close_to_float64 (targets inside and beyond reach), the largest reach error |tip - target| / (lab + lcb), and the
# first figure over the cases of one limb whose target lies ON the edge of reach. The host form calls no libm and reproduces exactly; the test
# asserts twice the measured value. The edge figure is of another order by nature, not by rounding alone: the sine of the angle at A is
# sqrt(reach - d) there, without a derivative, so d's last bit (1e-7) is 3e-4 of a bone length across the limb in ANY arithmetic.
F64_MEASURED = {"chain3": (7.858e-06, 2.144e-07, 9.971e-04), "chain70": (9.670e-05, 7.500e-08, 1.080e-03), "tree257": (3.079e-06, 2.243e-07, 4.001e-04),
                "tree1024": (2.658e-06, 1.547e-07, 1.463e-03)}
# The smallest margins the model met over those cases (asserted below, stated in the profile): 1 + dot from FRT_IK_ARC_EPS; decades between sin^2
# of the bend plane's angle and FRT_IK_PLANE_EPS; d from either end of the reach interval, as a fraction of the reach, for the targets not drawn on
# the edge; |c| from its clamp at 1 for the limbs whose reach was not clamped (a clamped reach puts c on the clamp by construction: counted, and
# harmless, since s is then exactly 0 whichever way c rounds); a length from 0; an aim slerp's |d| from 0.9995 and from 0. These are round lower
# bounds, one to two decades below the smallest margins the profile lists, so that another seed of the same generator passes too.
MARGINS = {"arc_margin": 1e-3, "plane_margin": 9.0, "reach_margin": 1e-3, "cos_margin": 1e-3, "length_margin": 1e-2, "ik_min_gap": 1e-3, "ik_min_abs_d": 0.1}


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def same(got, want):
    return [bits(x) for x in got] == [bits(x) for x in want]


def rig_of(frt, shape, **kw):
    desc = make_blend_rig(shape, nclips=3, **kw)
    return desc, frt.Rig(**desc)


def globals_of(rig, layers, masks=None, goals=None, targets=None):
    """float32 [N, 4, 4] column-major [c, r]: every node's global, read through evaluate_nodes_layers."""
    return rig.evaluate_nodes_layers(layers, np.arange(rig.num_nodes), masks=masks, goals=goals, targets=targets).reshape(-1, 4, 4)


def row(target, w=1.0, pole=None):
    return np.concatenate([target, [w], pole if pole is not None else np.zeros(3), [0.0 if pole is None else 1.0]]).astype(F)


STACK = [L(0, 0.4, 1.0), L(1, 0.5, 0.5, None, "override"), L(2, 0.6, 0.5, None, "additive", (2, 0.3))]


# ---------------------------------------------------------------------------------------------------------------- exact consequences
@pytest.mark.parametrize("shape", ("chain3", "tree257"))
def test_no_goals_zero_weights_and_skipped_goals_give_the_layered_bits(frt, shape):
    desc, rig = rig_of(frt, shape, joints="subset" if shape == "tree257" else "all")
    rng = np.random.default_rng(1)
    masks = random_masks(desc, 2, seed=1)
    nodes = np.arange(0, rig.num_nodes, 2)
    for rows_ in random_stacks(desc, 3, 2, "mixed", nmasks=2, seed=2):
        layers = to_layers(frt, rows_)
        want, want_nodes = rig.evaluate_layers(layers, masks), rig.evaluate_nodes_layers(layers, nodes, masks=masks)
        assert same(rig.evaluate_layers(layers, masks, [], None), want) and same(rig.evaluate_layers(layers, masks, None, None), want)
        goals = random_goals(desc, 6, rng)
        t = random_targets(desc, layered_globals(desc, rows_, masks)[0], goals, rng)
        zero = t.copy()
        zero[:, 3] = 0.0
        assert same(rig.evaluate_layers(layers, masks, to_goals(frt, goals), zero), want)
        assert bits(rig.evaluate_nodes_layers(layers, nodes, masks=masks, goals=to_goals(frt, goals), targets=zero)) == bits(want_nodes)
        assert not same(rig.evaluate_layers(layers, masks, to_goals(frt, goals), t), want)      # and with their weights they act
        # every goal skipped by the contract: a two-bone target at A itself (d = 0); an aim at the node's own origin
        glob = layered_globals(desc, rows_, masks)[0]
        skipped = [g for g in goals if isinstance(g, TB)][:1] + [g for g in goals if isinstance(g, AIM)][:1]
        f32 = globals_of(rig, layers, masks)
        at = np.stack([row(f32[g.root if isinstance(g, TB) else g.node][3, :3]) for g in skipped])
        assert same(rig.evaluate_layers(layers, masks, to_goals(frt, skipped), at), want), glob[0][3]


def test_nodes_outside_the_subtree_keep_their_bits(frt):
    desc, rig = rig_of(frt, "tree257")
    par = desc["parents"]
    rng = np.random.default_rng(3)
    layers = to_layers(frt, STACK)
    plain = globals_of(rig, layers)
    glob = layered_globals(desc, STACK)[0]
    for g in random_goals(desc, 12, rng):
        t = random_targets(desc, glob, [g], rng)
        got = globals_of(rig, layers, None, to_goals(frt, [g]), t)
        inside = subtree_flags(par, g.root if isinstance(g, TB) else g.node)
        assert bits(got[~inside]) == bits(plain[~inside]), g
        changed = np.array([bits(got[k]) != bits(plain[k]) for k in np.flatnonzero(inside)])
        assert changed.all(), g      # every node of the subtree moved (its origin or its axes)


def test_goals_act_in_list_order_each_on_what_the_earlier_left(frt):
    desc, rig = rig_of(frt, "chain70")
    layers = to_layers(frt, STACK)
    glob = layered_globals(desc, STACK)[0]
    arm, hand = TB(10, 14, 20), AIM(20, (0.0, 1.0, 0.0))      # a hand aim on the arm's tip, behind the arm's two-bone goal
    A = glob[10][3, :3]
    reach = np.linalg.norm(glob[14][3, :3] - A) + np.linalg.norm(glob[20][3, :3] - glob[14][3, :3])
    t = np.stack([row(A + 0.6 * reach * unit(np.array([0.3, -0.5, 0.8]))), row(A + np.array([2.0, 1.0, -1.0]))])
    both = globals_of(rig, layers, None, to_goals(frt, [arm, hand]), t)
    swapped = globals_of(rig, layers, None, to_goals(frt, [hand, arm]), t[::-1])
    assert bits(both) != bits(swapped)
    # the aim saw the arm's result: its pivot is the arm's target, and the hand's axis points from there at the aim's target
    assert np.abs(both[20][3, :3] - t[0, :3]).max() <= 1e-5 * reach
    axis = unit(both[20][1, :3].astype(D))
    assert np.abs(axis - unit(t[1, :3].astype(D) - both[20][3, :3])).max() <= 1e-5
    # and a second goal equals the first goal's result fed to a one-goal call: the model, goal by goal
    want = model_globals_ik(desc, STACK, None, [arm, hand], t)
    assert np.abs(both - np.stack(want)).max() <= 1e-4 * np.abs(np.stack(want)).max()


def bad_goals(nnodes, limb):
    """{what: [(kind, root, mid, tip, axis, reserved)]} each of which is refused; `limb` a valid TB of the rig."""
    ok = (0, limb.root, limb.mid, limb.tip, (0, 0, 0), 0)
    return {"an unknown kind": [ok, (2, 0, 0, 0, (0, 0, 1), 0)], "reserved != 0": [(0, limb.root, limb.mid, limb.tip, (0, 0, 0), 1)],
            "a root out of range": [(0, nnodes, limb.mid, limb.tip, (0, 0, 0), 0)], "a tip out of range": [ok, (0, limb.root, limb.mid, 0xFFFFFFFF, (0, 0, 0), 0)],
            "an aim node out of range": [(1, nnodes, 0, 0, (0, 0, 1), 0)], "mid is root": [(0, limb.root, limb.root, limb.tip, (0, 0, 0), 0)],
            "mid above root": [(0, limb.mid, limb.root, limb.tip, (0, 0, 0), 0)], "tip is mid": [(0, limb.root, limb.mid, limb.mid, (0, 0, 0), 0)],
            "tip above mid": [(0, limb.root, limb.tip, limb.mid, (0, 0, 0), 0)], "an aim axis of zero": [(1, 0, 0, 0, (0, 0, 0), 0)],
            "an aim axis NaN": [(1, 0, 0, 0, (0, np.nan, 1), 0)], "an aim axis inf": [ok, (1, 0, 0, 0, (np.inf, 0, 1), 0)],
            "an aim with a mid": [(1, limb.root, limb.mid, 0, (0, 0, 1), 0)], "an aim with a tip": [(1, limb.root, 0, limb.tip, (0, 0, 1), 0)]}


def bad_targets(good):
    """{what: float32 [2, 8]} each of which is refused for the goals [a two-bone goal, an aim]; `good` is accepted."""
    out = {}
    for what, (r_, c_, x) in {"a target NaN": (0, 1, np.nan), "a target inf": (1, 2, np.inf), "a weight NaN": (0, 3, np.nan), "a weight above 1": (1, 3, 1.0000001),
                              "a negative weight": (0, 3, -1e-30), "a pole NaN": (0, 5, np.nan), "a pole flag NaN": (0, 7, np.nan), "a pole flag of 2": (0, 7, 2.0),
                              "a pole flag of 0.5": (0, 7, 0.5), "a pole on an aim": (1, 7, 1.0), "a pole word on an aim": (1, 4, 0.25), "a pole flag -inf": (1, 7, -np.inf)}.items():
        t = np.array(good, F).copy()
        t[r_, c_] = x
        out[what] = t
    return out


def test_refusals_leave_the_outputs_untouched(frt):
    lib = frt.lib()
    desc, rig = rig_of(frt, "chain3", num_targets=3)
    G, S = frt.RigGoal, frt.ClipLayer
    limb = TB(0, 1, 2)
    layers = (S * 2)(S(0, 0.5, 1.0, 0xFFFFFFFF, 0, 0, 0.0, 0), S(1, 0.5, 0.5, 0xFFFFFFFF, 1, 0, 0.0, 0))
    nodes = np.array([2, 0, 1], np.uint32)
    pal, w, mats = np.full((3, 16), 7.0, F), np.full(3, 7.0, F), np.full((3, 16), 7.0, F)
    good_t = np.stack([row(np.array([0.2, 0.3, 0.1]), 1.0, np.array([0.0, 1.0, 0.0])), row(np.array([1.0, 0.5, 0.2]), 0.5)])

    def table(rows_):
        return (G * max(len(rows_), 1))(*[G(k, a, m, t, (C.c_float * 3)(*ax), res) for k, a, m, t, ax, res in rows_])

    def both(ng, goals, targets):
        g = None if goals is None else table(goals)
        t = None if targets is None else np.ascontiguousarray(targets, F)
        tp = None if t is None else t.ctypes.data
        a = lib.frt_rig_evaluate_layers_ik(rig._h, 2, layers, 0, None, ng, g, tp, pal.ctypes.data, w.ctypes.data)
        assert a != -1 or b"rig_evaluate_layers_ik" in lib.frt_last_error()
        return a, lib.frt_rig_evaluate_nodes_layers_ik(rig._h, 2, layers, 0, None, ng, g, tp, 3, nodes.ctypes.data, None, None, mats.ctypes.data)

    ok = [(0, 0, 1, 2, (0, 0, 0), 0), (1, 2, 0, 0, (0, 0, 1), 0)]
    for what, rows_ in bad_goals(3, limb).items():
        t = np.tile(row(np.array([0.2, 0.3, 0.1])), (len(rows_), 1))
        assert both(len(rows_), rows_, t) == (-1, -1), what
    for what, t in bad_targets(good_t).items():
        assert both(2, ok, t) == (-1, -1), what
    assert both(17, ok * 9, np.tile(good_t, (9, 1))) == (-1, -1)          # more than FRT_MAX_RIG_GOALS, before anything is read
    assert both(0xFFFFFFFF, ok, good_t) == (-1, -1)
    assert both(2, None, good_t) == (-1, -1) and both(2, ok, None) == (-1, -1)      # null arrays with a count
    bad_layers = (S * 1)(S(0, 0.5, 0.0, 0xFFFFFFFF, 0, 0, 0.0, 0))         # what the layered call refuses is refused here
    assert lib.frt_rig_evaluate_layers_ik(rig._h, 1, bad_layers, 0, None, 2, table(ok), good_t.ctypes.data, pal.ctypes.data, w.ctypes.data) == -1
    assert lib.frt_rig_evaluate_layers_ik(None, 2, layers, 0, None, 2, table(ok), good_t.ctypes.data, pal.ctypes.data, w.ctypes.data) == -1
    assert lib.frt_rig_evaluate_layers_ik(rig._h, 2, layers, 0, None, 2, table(ok), good_t.ctypes.data, None, w.ctypes.data) == -1
    assert (pal == 7.0).all() and (w == 7.0).all() and (mats == 7.0).all()
    assert both(2, ok, good_t) == (0, 0) and not (pal == 7.0).any() and not (mats == 7.0).any()      # and the good call writes
    assert both(0, None, None) == (0, 0)                                                            # no goals: the layered call
    assert bits(pal) == bits(rig.evaluate_layers([(0, 0.5, 1.0), frt.Layer(1, 0.5, 0.5, mode="override")])[0])
    for goals, t in (([frt.TwoBone(0, 1, 2)], None), ([frt.TwoBone(0, 1, 2)], np.zeros((2, 8), F)), ([frt.TwoBone(0, 1, 2)], np.zeros((1, 7), F)), ([(0, 1, 2)], np.zeros((1, 8), F)),
                     ([frt.Aim(0, (0, 1))], np.zeros((1, 8), F)), ([frt.Aim(0)] * 17, np.zeros((17, 8), F))):
        with pytest.raises(frt.FrtError):
            rig.evaluate_layers([(0, 0.5, 1.0)], None, goals, t)


# ---------------------------------------------------------------------------------------------------------------- behaviour
def _limb_world(frt):
    desc, rig = rig_of(frt, "chain70")
    layers = to_layers(frt, STACK)
    g = TB(30, 33, 37)      # nodes between root, mid and tip are carried rigidly
    plain = globals_of(rig, layers).astype(D)
    A, B, Cc = plain[30][3, :3], plain[33][3, :3], plain[37][3, :3]
    return desc, rig, layers, g, A, B, Cc, np.linalg.norm(B - A), np.linalg.norm(Cc - B)


def test_a_reachable_target_is_reached_with_the_bone_lengths_kept(frt):
    desc, rig, layers, g, A, B, Cc, lab, lcb = _limb_world(frt)
    rng = np.random.default_rng(4)
    for k in range(8):
        T = A + rng.uniform(max(abs(lab - lcb) / (lab + lcb) + 0.05, 0.3), 0.95) * (lab + lcb) * unit(rng.standard_normal(3))
        got = globals_of(rig, layers, None, to_goals(frt, [g]), row(T)[None, :]).astype(D)
        A1, B1, C1 = got[30][3, :3], got[33][3, :3], got[37][3, :3]
        # float32 roundings of values of the limb's size: a few 2^-24 of the reach each, through two rotations and the layered globals
        tol = 64 * 2.0 ** -24 * max(lab + lcb, np.abs(A).max())
        assert np.abs(A1 - A).max() <= tol and np.abs(C1 - T).max() <= tol, k
        assert abs(np.linalg.norm(B1 - A1) - lab) <= tol and abs(np.linalg.norm(C1 - B1) - lcb) <= tol, k


def test_an_unreachable_target_straightens_the_limb_towards_it(frt):
    desc, rig, layers, g, A, B, Cc, lab, lcb = _limb_world(frt)
    rng = np.random.default_rng(5)
    for k in range(6):
        dr = unit(rng.standard_normal(3))
        got = globals_of(rig, layers, None, to_goals(frt, [g]), row(A + rng.uniform(1.2, 3.0) * (lab + lcb) * dr)[None, :]).astype(D)
        B1, C1 = got[33][3, :3], got[37][3, :3]
        assert np.abs(C1 - (A + (lab + lcb) * dr)).max() <= 64 * 2.0 ** -24 * max(lab + lcb, np.abs(A).max()), k
        # c = 1 to a few roundings e <= 4 x 2^-24, so s = sqrt(1 - c c) <= sqrt(2 e) = 7e-4: B' lies that fraction of lab off the line
        assert np.linalg.norm(np.cross(B1 - A, dr)) <= 1e-3 * lab and (B1 - A) @ dr > 0.999 * lab, k


def test_the_bend_faces_the_pole(frt):
    desc, rig, layers, g, A, B, Cc, lab, lcb = _limb_world(frt)
    rng = np.random.default_rng(6)
    for k in range(8):
        dr = unit(rng.standard_normal(3))
        T = A + 0.6 * (lab + lcb) * dr
        P = A + rng.standard_normal(3)
        side = (P - A) - ((P - A) @ dr) * dr      # the pole's side of the line A -> T
        if np.linalg.norm(side) < 0.2:
            continue
        got = globals_of(rig, layers, None, to_goals(frt, [g]), row(T, 1.0, P)[None, :]).astype(D)
        B1 = got[33][3, :3]
        off = (B1 - A) - ((B1 - A) @ dr) * dr
        assert off @ side > 0.0 and np.linalg.norm(np.cross(unit(off), unit(side))) <= 1e-4, k      # in the plane of dir and the pole, on the pole's side


def test_an_aim_points_its_axis_at_the_target_and_half_way_at_half_weight(frt):
    desc, rig, layers, g, A, B, Cc, lab, lcb = _limb_world(frt)
    plain = globals_of(rig, layers).astype(D)
    rng = np.random.default_rng(7)
    for k in range(6):
        axis = unit(rng.standard_normal(3)).astype(F)
        node = int(rng.integers(0, 70))
        O = plain[node][3, :3]
        cur = unit(plain[node][0, :3] * axis[0] + plain[node][1, :3] * axis[1] + plain[node][2, :3] * axis[2])
        T = O + 2.0 * unit(rng.standard_normal(3))
        want = unit(np.asarray(T, F).astype(D) - O)
        full = np.arccos(np.clip(cur @ want, -1, 1))
        for w in (1.0, 0.5):
            got = globals_of(rig, layers, None, [frt.Aim(node, axis)], row(T, w)[None, :]).astype(D)
            now = unit(got[node][0, :3] * axis[0] + got[node][1, :3] * axis[1] + got[node][2, :3] * axis[2])
            assert np.abs(got[node][3, :3] - O).max() <= 16 * 2.0 ** -24 * max(1.0, np.abs(O).max())      # the pivot stays
            assert abs(np.arccos(np.clip(now @ want, -1, 1)) - (1.0 - w) * full) <= 2e-3      # (arccos near 0 amplifies 1e-7 to 5e-4)
            assert abs(np.arccos(np.clip(now @ cur, -1, 1)) - w * full) <= 2e-3


# ---------------------------------------------------------------------------------------------------------------- accuracy
def ik_cases(desc, shape):
    """[(layer rows, masks, goals, targets)]: 1, 2 and 16 goals of both kinds over a 1-layer and a 3-layer masked pose; targets inside, on the edge
    of and beyond reach, chained and overlapping as the hierarchy makes them."""
    rng = np.random.default_rng(len(shape) + 100)
    masks = random_masks(desc, 4, seed=len(shape))
    out = []
    for nl in (1, 3):
        rows_ = random_stacks(desc, nl, 1, "mixed", nmasks=4, seed=nl)[0]
        seen = {}      # the decisions of the layers' own slerps
        glob = layered_globals(desc, rows_, masks, seen)[0]
        for ng in GOAL_COUNTS:      # targets inside and beyond reach, chained and overlapping
            goals = random_goals(desc, ng, rng)
            out.append((rows_, masks, goals, random_targets(desc, glob, goals, rng), glob, seen, "chained"))
        for _ in range(3):          # a target ON the edge of reach: one limb a case, nothing stacked on it
            goals = random_goals(desc, 1, rng, kinds="two_bone")
            out.append((rows_, masks, goals, random_targets(desc, glob, goals, rng, reach="edge"), glob, seen, "edge"))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_goals_are_close_to_float64(frt, shape):
    """No case is left out; every threshold decision of the model is clear of its threshold by the margins asserted here. The layers' own slerps
    meet d > 0.9995 arbitrarily closely, as in test_animation_layers.py: the branch gap of 5.1e-7 lies inside every bound."""
    desc, rig = rig_of(frt, shape)
    flip = threshold_branch_gap()
    assert 4.5e-7 < flip < 5.5e-7 and flip < 2 * F64_MEASURED[shape][0]
    met, worst, reach, kinds = {}, {"chained": 0.0, "edge": 0.0}, 0.0, set()
    for rows_, masks, goals, t, glob, seen, tag in ik_cases(desc, shape):
        layers, fg = to_layers(frt, rows_), to_goals(frt, goals)
        met["min_abs_d"] = min(met.get("min_abs_d", 1.0), seen.get("min_abs_d", 1.0))
        pal, w = rig.evaluate_layers(layers, masks, fg, t)
        mg = model_globals_ik(desc, rows_, masks, goals, t, met, glob)
        from _ik_model import palette_of
        mp = palette_of(desc, mg)
        worst[tag] = max(worst[tag], float(np.abs(pal - mp).max() / np.abs(mp).max()))
        nodes = np.arange(0, rig.num_nodes, 3)
        mats = rig.evaluate_nodes_layers(layers, nodes, masks=masks, goals=fg, targets=t)
        mm = np.stack([mg[k].reshape(16) for k in nodes])
        worst[tag] = max(worst[tag], float(np.abs(mats - mm).max() / np.abs(mm).max()))
        g, r_ = goals[-1], t[-1]      # the last goal's tip is moved by no later goal: its reach error, where the target can be reached at full weight
        if isinstance(g, TB) and r_[3] == 1.0:
            before = model_globals_ik(desc, rows_, masks, goals[:-1], t[:-1], None, glob)
            A, B, Cc = (before[i][3, :3] for i in g)
            lab, lcb = np.linalg.norm(B - A), np.linalg.norm(Cc - B)
            if abs(lab - lcb) <= np.linalg.norm(r_[:3] - A) <= (lab + lcb) * (1 - 1e-6):
                tip = rig.evaluate_nodes_layers(layers, [g.tip], masks=masks, goals=fg, targets=t)[0, 12:15]
                reach = max(reach, float(np.linalg.norm(tip - r_[:3]) / (lab + lcb)))
        kinds |= {type(x).__name__ for x in goals}
    print(f"{shape}: max |f32 - f64| / max |f64| = {worst['chained']:.3e}, on the edge of reach {worst['edge']:.3e}; reach error = {reach:.3e}; " + "; ".join(f"{k} = {met[k]:.3e}" for k in MARGINS if k in met) +
          f"; inside / edge / beyond / short = {met.get('reach_inside', 0)} / {met.get('reach_on_edge', 0)} / {met.get('reach_beyond', 0)} / {met.get('reach_short', 0)}; "
          f"c on its clamp {met.get('cos_on_clamp', 0)}; records applied {met.get('applied_records', 0)}, skipped {met.get('skipped_record', 0)}; pole fallbacks {met.get('pole_fallbacks', 0)}; half turns {met.get('arc_half_turns', 0)}")
    assert kinds == {"TB", "AIM"} and met.get("reach_beyond", 0) and met.get("reach_on_edge", 0) and met.get("reach_inside", 0)
    assert not any(met.get(k, 0) for k in ("skipped_record", "skipped_zero_length", "skipped_no_plane", "pole_fallbacks", "arc_half_turns"))
    for k, least in MARGINS.items():
        assert met[k] >= least, (k, met[k])
    assert met["min_abs_d"] > 0.5      # the layers' slerps: no sign decision near 0
    clamped = met.get("reach_beyond", 0) + met.get("reach_short", 0)      # c sits on its clamp where lat was clamped (and where d is an end itself)
    assert clamped <= met.get("cos_on_clamp", 0) <= clamped + met.get("reach_on_edge", 0)
    assert worst["chained"] <= 2 * F64_MEASURED[shape][0], worst
    assert reach <= 2 * F64_MEASURED[shape][1], reach
    assert worst["edge"] <= 2 * F64_MEASURED[shape][2], worst


def test_the_degenerate_branches_take_the_models_decisions(frt):
    """Deterministic inputs, a rig whose layered pose is exact in float32 (an L of unit bones, no rotation), the host form's decision against the
    model's: skipped means the layered bits, taken means the model's result."""
    par = np.array([-1, 0, 1, 2], np.int32)
    tr = np.array([[0, 0, 0], [0, 1, 0], [0, 0.5, 0], [0, 0, 0]], F)      # a straight limb 0 - 1 - 2 along y, bones of 1 and 0.5; node 3 sits on node 2 (a zero-length bone)
    desc = {"parents": par, "translations": tr, "joint_nodes": np.arange(4, dtype=np.uint32), "clips": [("rest", [])]}
    rig = frt.Rig(**desc)
    layers, rows_ = [("rest", 0.0, 1.0)], [L(0, 0.0, 1.0)]
    plain = rig.evaluate_layers(layers)[0]
    x, y, z = np.eye(3)
    cases = {"a straight limb without a pole has no bend plane": ([TB(0, 1, 2)], [row(1.5 * y)], "skipped_no_plane"),
             "a straight limb, an off-line target: the limb gives the plane": ([TB(0, 1, 2)], [row(1.2 * unit(x + y))], None),
             "a straight limb with a pole bends towards it": ([TB(0, 1, 2)], [row(1.2 * y, 1.0, x)], None),
             "a pole on the line falls back to the limb, which is on it too": ([TB(0, 1, 2)], [row(1.5 * y, 1.0, 3.0 * y)], "skipped_no_plane"),
             "a pole on the line to an off-line target falls back to the limb": ([TB(0, 1, 2)], [row(1.2 * x, 1.0, 2.0 * x)], "pole_fallbacks"),
             "an antiparallel aim is a half turn": ([AIM(1, (0.0, 1.0, 0.0))], [row(-3.0 * y)], "arc_half_turns"),
             "a target at A": ([TB(0, 1, 2)], [row(0.0 * y)], "skipped_zero_length"), "an aim at its own origin": ([AIM(1, (1.0, 0.0, 0.0))], [row(y)], "skipped_zero_length"),
             "a zero-length bone": ([TB(1, 2, 3)], [row(x)], "skipped_zero_length"),
             "a target inside |lab - lcb| = 0.5 folds the limb back on itself, the tip at 0.5": ([TB(0, 1, 2)], [row(0.2 * x, 1.0, z)], "reach_short"),
             "a target beyond lab + lcb = 1.5 stretches it": ([TB(0, 1, 2)], [row(4.0 * unit(x + z), 1.0, y)], "reach_beyond")}
    for what, (goals, t, decision) in cases.items():
        t = np.stack(t)
        met = {}
        mp, _ = model_evaluate_layers_ik(desc, rows_, None, goals, t, met)
        got = rig.evaluate_layers(layers, None, to_goals(frt, goals), t)[0]
        skipped = any(k.startswith("skipped") for k in met)
        assert (decision is None or met.get(decision, 0) >= 1) and skipped == (decision is not None and decision.startswith("skipped")), (what, met)
        assert (bits(got) == bits(plain)) == skipped, what
        assert np.abs(got - mp).max() <= 1e-5, what      # (values of size one, a dozen roundings; a clamped reach is exact: s = 0)


def test_symbols_are_exported(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for text in ("#define FRT_MAX_RIG_GOALS 16u", "enum { FRT_GOAL_TWO_BONE = 0, FRT_GOAL_AIM = 1 };", "#define FRT_IK_PLANE_EPS 1e-12f", "#define FRT_IK_ARC_EPS 1e-6f",
                 "#define FRT_GOAL_TARGETS_DEVICE 1u", "typedef struct frt_rig_goal { uint32_t kind, root, mid, tip; float axis[3]; uint32_t reserved; } frt_rig_goal;",
                 "typedef struct frt_rig_goal_target { float target[3], weight, pole[3], pole_flag; } frt_rig_goal_target;"):
        assert text in header, text
    lib = frt.lib()
    for name in ("frt_rig_evaluate_layers_ik", "frt_rig_evaluate_nodes_layers_ik", "frt_renderer_set_rig_goals", "frt_renderer_set_rig_goal_targets"):
        assert hasattr(lib, name) and name + "(" in header, name
    assert C.sizeof(frt.RigGoal) == 32 and C.sizeof(frt.RigGoalTarget) == 32 and (frt.MAX_RIG_GOALS, frt.GOAL_TARGETS_DEVICE) == (16, 1)
    assert frt.GOAL_KINDS == {"two_bone": 0, "aim": 1}
    for cls in (frt.SceneBuilder, frt.MultiRenderer):
        for call in ("animate_layers", "animate_instances_layers"):
            assert "goals" in getattr(cls, call).__code__.co_varnames and "targets" in getattr(cls, call).__code__.co_varnames, (cls, call)
    assert callable(frt.Renderer.set_rig_goals) and callable(frt.Renderer.set_rig_goal_targets) and repr(frt.TwoBone(0, 1, 2)) and frt.Aim(3).axis == (0, 0, 1)
    assert lib.frt_renderer_set_rig_goals(None, 0, 0, None) == -1 and b"set_rig_goals" in lib.frt_last_error()      # a null renderer, before anything else
    assert lib.frt_renderer_set_rig_goal_targets(None, 0, 0, None, 0) == -1 and b"set_rig_goal_targets" in lib.frt_last_error()


def test_scene_forms_are_the_host_evaluation_then_the_host_calls(frt):
    from test_mesh_deform import CUBE, SPHERE, EVERYTHING
    from test_instance_update import cornell_meshes
    from _skin_model import make_skin
    meshes = cornell_meshes(frt)
    ids = [CUBE, SPHERE]
    desc = make_blend_rig("tree12", nclips=3, seed=3, joints="subset", num_targets=0, keys=(2, 5), spread=0.2)
    desc["translations"] = F(0.1) * desc["translations"]
    rig = frt.Rig(**desc)
    a, b = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    for s in (a, b):
        for m in ids:
            s.set_mesh_skin(m, *make_skin(len(meshes[m].positions), rig.num_joints, seed=m), num_joints=rig.num_joints)
    goals = [frt.Aim(2, (0, 1, 0)), frt.Aim(5)]
    t = np.stack([row(np.array([0.3, 0.2, 0.1]), 0.5), row(np.array([-0.2, 0.4, 0.3]))])
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    a.animate_layers(rig, ids, layers, goals=goals, targets=t)
    b.set_mesh_poses(ids, *rig.evaluate_layers(layers, None, goals, t))
    a.animate_cast_layers([{"rig": rig, "mesh_ids": ids, "layers": layers, "goals": goals, "targets": t}], normals="keep")
    b.animate_layers(rig, ids, layers, None, "keep", goals, t)
    for w in EVERYTHING:
        assert a.get(w).tobytes() == b.get(w).tobytes(), w
    prig = frt.Rig(**dict(desc, joint_nodes=(), inverse_bind=None), nodes_only=True)
    a.animate_instances_layers(prig, [1, 0], [3, 7], layers, goals=goals, targets=t)
    b.set_instance_transforms([1, 0], prig.evaluate_nodes_layers(layers, [3, 7], goals=goals, targets=t))
    for w in EVERYTHING:
        assert a.get(w).tobytes() == b.get(w).tobytes(), w


def test_host_forms_run_clean_under_a_sanitiser(tmp_path):
    """tools/ik_sanitize.cpp with csrc/frt_animation.cpp, stand-alone, with -fsanitize=address,undefined (the command line of layers_sanitize)."""
    exe = str(tmp_path / "ik_sanitize")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math"] + san +
                   [os.path.join(ROOT, "tools", "ik_sanitize.cpp"), os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc", "frt_animation.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok: "), run.stdout + run.stderr
