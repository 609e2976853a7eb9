"""What the chain-IK tests share (include/frt.h: FRT_GOAL_CHAIN; DESIGN.md section 11, "Chain IK"): a float64 restatement of the chain contract,
written from the contract over tests/_ik_model.py's arc / about / point helpers (it calls nothing of the library), and chain goals with targets in
general position. A model chain goal is a CH(root, tip, sweeps) in the description's node numbers; TB and AIM goals of _ik_model may stand beside
it in one list. Every decision a chain meets is recorded in `met`: per step the two zero-length tests (`chain_length_margin`: the smaller of |e|
and |t| as a fraction of the chain's reach) and ik_arc's 1 + dot < FRT_IK_ARC_EPS (`arc_margin`, `arc_half_turns`, by _ik_model.arc)."""
from collections import namedtuple
import numpy as np
from _anim_model import F, D, mat_mul
from _ik_model import TB, AIM, note, count, unit, arc, about, point, target_ok, subtree_flags, apply_goal, layered_globals, palette_of, random_targets

CH = namedtuple("CH", "root tip sweeps", defaults=(8,))
MAX_NODES, MAX_SWEEPS = 32, 16      # FRT_IK_CHAIN_MAX_NODES, FRT_IK_CHAIN_MAX_SWEEPS


def to_goals(frt, goals):
    return [frt.Chain(g.root, g.tip, g.sweeps) if isinstance(g, CH) else (frt.TwoBone(*g) if isinstance(g, TB) else frt.Aim(g.node, g.axis)) for g in goals]


def chain_nodes(parents, root, tip):
    """[c_0 = root, ..., c_K = tip]: the parent path."""
    path = [int(tip)]
    while path[-1] != root:
        p = int(parents[path[-1]])
        assert p >= 0, "tip is not below root"
        path.append(p)
    return path[::-1]


def chain_reach(P):
    return float(sum(np.linalg.norm(P[j + 1] - P[j]) for j in range(len(P) - 1)))


def solve_chain(P, Te, sweeps, met=None):
    """(P after the sweeps, [D_0 .. D_K]) of the origins P [K + 1, 3] under the effective target Te."""
    P = [np.array(p, D) for p in P]
    K = len(P) - 1
    reach = chain_reach(P)
    Ds = [np.eye(4) for _ in range(K + 1)]
    for _ in range(sweeps):
        for k in range(K - 1, -1, -1):
            e, t = P[K] - P[k], Te - P[k]
            le, lt = np.sqrt(e @ e), np.sqrt(t @ t)
            note(met, "chain_length_margin", min(le, lt) / reach if reach > 0.0 else 0.0)
            count(met, "chain_steps")
            if not (le > 0.0 and lt > 0.0):
                count(met, "chain_steps_skipped")
                continue
            R = about(P[k], arc(unit(e), unit(t), met))
            for j in range(k + 1, K + 1):
                P[j] = point(R, P[j])
            for j in range(k, K + 1):
                Ds[j] = mat_mul(R, Ds[j])
    return P, Ds


def effective_target(tip, row):
    return row[:3] if row[3] == 1.0 else tip + row[3] * (row[:3] - tip)


def apply_chain(parents, glob, goal, row, met=None):
    """The globals (a list of [4, 4], the description's node order) after one chain goal; `glob` is not changed."""
    row = np.asarray(row, F).astype(D)
    if not target_ok(row):
        count(met, "skipped_record")
        return glob
    count(met, "applied_records")
    c = chain_nodes(parents, goal.root, goal.tip)
    K = len(c) - 1
    P = [glob[n][3, :3] for n in c]
    _, Ds = solve_chain(P, effective_target(P[K], row), goal.sweeps, met)
    out = list(glob)
    deepest = np.full(len(parents), -1)
    for j, n in enumerate(c):      # nested subtrees: the later, the deeper
        deepest[subtree_flags(parents, n)] = j
    for n in np.flatnonzero(deepest >= 0):
        out[n] = mat_mul(Ds[min(deepest[n], K - 1)], glob[n])      # the tip's own subtree moves with the last bone
    return out


def apply_any(parents, glob, goal, row, met=None):
    return apply_chain(parents, glob, goal, row, met) if isinstance(goal, CH) else apply_goal(parents, glob, goal, row, met)


def model_globals(desc, layers, masks, goals, targets, met=None, glob=None):
    glob = layered_globals(desc, layers, masks)[0] if glob is None else glob
    for g, row in zip(goals, np.asarray(targets, F).reshape(-1, 8)):
        glob = apply_any(desc["parents"], glob, g, row, met)
    return glob


def model_palette(desc, glob):
    return palette_of(desc, glob)


def chain_target(glob, parents, goal, rng, frac=(0.3, 0.9), w=1.0):
    """A float32 target row for a chain on the globals `glob`: at `frac` of the chain's reach from its root's origin, in a random direction."""
    c = chain_nodes(parents, goal.root, goal.tip)
    P = [glob[n][3, :3] for n in c]
    T = P[0] + rng.uniform(*frac) * chain_reach(P) * unit(rng.standard_normal(3))
    return np.concatenate([T, [w], rng.standard_normal(3), [float(rng.integers(0, 2))]]).astype(F)      # (the pole words are ignored: anything finite)


def mixed_targets(desc, glob, goals, rng, weights=(1.0, 0.5, None)):
    """float32 [G, 8] for a list of CH, TB and AIM goals, drawn goal by goal on the model's own result of the goals before it; weights 1, 0.5 and
    random in turn for the chains, _ik_model.random_targets' for the others."""
    rows = np.zeros((len(goals), 8), F)
    for k, g in enumerate(goals):
        if isinstance(g, CH):
            w = weights[k % len(weights)]
            rows[k] = chain_target(glob, desc["parents"], g, rng, w=float(F(rng.uniform(0.2, 0.95))) if w is None else w)
        else:
            rows[k] = random_targets(desc, glob, [g], rng)[0]
        glob = apply_any(desc["parents"], glob, g, rows[k])
    return rows
