"""What the inverse-kinematics tests share (include/frt.h: frt_rig_evaluate_layers_ik; DESIGN.md section 11, "Inverse kinematics"): a float64
restatement of the goal contract over tests/_anim_model.py's matrices and slerp and tests/_layers_model.py's layered pose, written from the contract
(it calls nothing of the library), and goals with targets drawn so that, in this model, no threshold decision lies near its threshold. A model goal
is a TB(root, mid, tip) or an AIM(node, axis) in the description's node numbers; targets are float32 [G, 8] rows of (target xyz, weight, pole xyz,
pole flag). Matrices are column-major [c, r] as in _anim_model. Every decision a goal meets is recorded in `met` (see note())."""
from collections import namedtuple
import numpy as np
from _anim_model import F, D, slerp, trs_matrix, mat_mul
from _layers_model import model_evaluate_layers, _note

TB = namedtuple("TB", "root mid tip")
AIM = namedtuple("AIM", "node axis", defaults=((0.0, 0.0, 1.0),))
PLANE_EPS, ARC_EPS = D(F(1e-12)), D(F(1e-6))      # FRT_IK_PLANE_EPS, FRT_IK_ARC_EPS as the float32 constants they are
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0], D)


def to_goals(frt, goals):
    return [frt.TwoBone(*g) if isinstance(g, TB) else frt.Aim(g.node, g.axis) for g in goals]


def note(met, key, value):
    """met[key] keeps the smallest value seen; met["n_" + key] counts."""
    if met is not None:
        met[key] = min(met.get(key, np.inf), float(value))
        met["n_" + key] = met.get("n_" + key, 0) + 1


def count(met, key):
    if met is not None:
        met[key] = met.get(key, 0) + 1


def unit(v):
    return v / np.sqrt(np.dot(v, v))


def arc(u, v, met=None):
    d = 1.0 + np.dot(u, v)
    note(met, "arc_margin", abs(d - ARC_EPS))      # the antiparallel decision: how far 1 + dot lies from FRT_IK_ARC_EPS
    if d < ARC_EPS:
        count(met, "arc_half_turns")
        a = np.abs(u)
        e = np.eye(3)[0 if a[0] <= a[1] and a[0] <= a[2] else (1 if a[1] <= a[2] else 2)]
        return np.append(unit(np.cross(u, e)), 0.0)
    q = np.append(np.cross(u, v), d)
    return q / np.sqrt(np.dot(q, q))


def about(p, q):
    m = trs_matrix(np.zeros(3), q, np.ones(3))
    m[3, :3] = p - (m[0, :3] * p[0] + m[1, :3] * p[1] + m[2, :3] * p[2])
    return m


def point(m, p):
    return m[0, :3] * p[0] + m[1, :3] * p[1] + m[2, :3] * p[2] + m[3, :3]


def target_ok(row):
    w = row[3]
    return bool(np.all(np.isfinite(row)) and w > 0.0 and w <= 1.0)


def two_bone(A, B, C, row, met=None):
    """(Da, Db Da) or None when the goal is skipped."""
    T, w, P, pole = row[:3], row[3], row[4:7], row[7] != 0.0
    Te = T if w == 1.0 else C + w * (T - C)
    ab, cb, at = B - A, C - B, Te - A
    lab, lcb, d = np.sqrt(ab @ ab), np.sqrt(cb @ cb), np.sqrt(at @ at)
    note(met, "length_margin", min(lab, lcb, d))      # the second skip test: a length that is not > 0
    if not (lab > 0.0 and lcb > 0.0 and d > 0.0):
        count(met, "skipped_zero_length")
        return None
    direction = at / d
    lo, hi = abs(lab - lcb), lab + lcb
    # the reach clamp: how far d lies from either end of [|lab - lcb|, lab + lcb]. A target ON the edge (within 1e-6 of it: the "edge" targets, drawn
    # there on purpose) is counted instead: min and max are continuous, so either side of that decision gives the same lat to rounding
    edge = min(abs(d - lo), abs(d - hi)) / hi
    if edge < 1e-6:
        count(met, "reach_on_edge")
    else:
        note(met, "reach_margin", edge)
    count(met, "reach_beyond" if d > hi else ("reach_short" if d < lo else "reach_inside"))
    lat = min(max(d, lo), hi)
    side = P - A if pole else ab
    nrm = np.cross(direction, side)

    def plane_ok(nrm, side):
        s2 = side @ side
        ratio = (nrm @ nrm) / s2 if s2 > 0.0 else 0.0
        note(met, "plane_margin", abs(np.log10(ratio / PLANE_EPS)) if ratio > 0.0 else np.inf)      # decades between sin^2 and FRT_IK_PLANE_EPS
        return nrm @ nrm > PLANE_EPS * s2

    if not plane_ok(nrm, side):
        if not pole:
            count(met, "skipped_no_plane")
            return None
        count(met, "pole_fallbacks")
        side = ab
        nrm = np.cross(direction, side)
        if not plane_ok(nrm, side):
            count(met, "skipped_no_plane")
            return None
    perp = np.cross(unit(nrm), direction)
    c = (lab * lab + lat * lat - lcb * lcb) / (2.0 * lab * lat)
    # the clamp of c to [-1, 1]: a clamped lat puts c ON the clamp (c = +-1 to rounding; counted, and harmless: s below does not depend on c and
    # is exactly 0 there); for every other limb how far |c| lies from 1
    if lat in (lo, hi):
        count(met, "cos_on_clamp")
    elif edge < 1e-6:
        count(met, "cos_on_edge")      # (a target drawn on the edge of reach that fell just inside it: |c| is 1 to 1e-6, by design)
    else:
        note(met, "cos_margin", 1.0 - abs(c))
    c = min(max(c, -1.0), 1.0)
    s = np.sqrt(max((lat + (lcb - lab)) * ((lab + lcb) - lat) * (lat + (lab - lcb)) * ((lab + lcb) + lat), 0.0)) / (2.0 * lab * lat)
    B1 = A + lab * (c * direction + s * perp)
    C2 = A + lat * direction
    da = about(A, arc(unit(ab), unit(B1 - A), met))
    C1 = point(da, C)
    db = about(B1, arc(unit(C1 - B1), unit(C2 - B1), met))
    return da, mat_mul(db, da)


def aim(G, axis, row, met=None):
    O = G[3, :3]
    v = G[0, :3] * axis[0] + G[1, :3] * axis[1] + G[2, :3] * axis[2]
    to = row[:3] - O
    note(met, "length_margin", min(np.sqrt(v @ v), np.sqrt(to @ to)))
    if not (np.sqrt(v @ v) > 0.0 and np.sqrt(to @ to) > 0.0):
        count(met, "skipped_zero_length")
        return None
    q = arc(unit(v), unit(to), met)
    if row[3] < 1.0:
        sm = {}
        _note(sm, IDENTITY, q)      # the slerp's two decisions: the sign of the dot product and d > 0.9995
        if met is not None:
            met["ik_min_abs_d"] = min(met.get("ik_min_abs_d", 1.0), sm["min_abs_d"])
            met["ik_min_gap"] = min(met.get("ik_min_gap", 1.0), sm["min_gap"])
        q = slerp(IDENTITY, q, row[3])
    return about(O, q)


def subtree_flags(parents, root):
    inside = np.zeros(len(parents), bool)
    inside[root] = True
    for n, p in enumerate(parents):
        if p >= 0 and inside[p]:
            inside[n] = True
    return inside


def apply_goal(parents, glob, goal, row, met=None):
    """The globals (a list of [4, 4], the description's node order) after one goal; `glob` is not changed."""
    row = np.asarray(row, F).astype(D)
    if not target_ok(row):      # the first skip test
        count(met, "skipped_record")
        return glob
    count(met, "applied_records")
    out = list(glob)
    if isinstance(goal, AIM):
        d = aim(glob[goal.node], np.asarray(goal.axis, F).astype(D), row, met)
        if d is None:
            return glob
        for n in np.flatnonzero(subtree_flags(parents, goal.node)):
            out[n] = mat_mul(d, glob[n])
        return out
    r = two_bone(glob[goal.root][3, :3], glob[goal.mid][3, :3], glob[goal.tip][3, :3], row, met)
    if r is None:
        return glob
    inner = subtree_flags(parents, goal.mid)
    for n in np.flatnonzero(subtree_flags(parents, goal.root)):
        out[n] = mat_mul(r[1] if inner[n] else r[0], glob[n])
    return out


def layered_globals(desc, layers, masks=None, met=None):
    """The layered pose's globals, a list of [4, 4] float64, and the morph weights: model_evaluate_layers of the description with every node a
    joint under an identity inverse bind matrix."""
    n = len(desc["parents"])
    every = dict(desc, joint_nodes=np.arange(n, dtype=np.uint32), inverse_bind=None)
    pal, w = model_evaluate_layers(every, layers, masks, met)
    return [pal[k].reshape(4, 4) for k in range(n)], w


def palette_of(desc, glob):
    joints = np.asarray(desc.get("joint_nodes", ()), np.int64)
    if not joints.size:
        return None
    ib = desc.get("inverse_bind")
    ib = np.tile(np.eye(4).reshape(16), (joints.size, 1)) if ib is None else np.asarray(ib, F).astype(D).reshape(-1, 16)
    return np.stack([mat_mul(glob[j], ib[k].reshape(4, 4)).reshape(16) for k, j in enumerate(joints)])


def model_globals_ik(desc, layers, masks, goals, targets, met=None, glob=None):
    glob = layered_globals(desc, layers, masks, met)[0] if glob is None else glob
    for g, row in zip(goals, np.asarray(targets, F).reshape(-1, 8)):
        glob = apply_goal(desc["parents"], glob, g, row, met)
    return glob


def model_evaluate_layers_ik(desc, layers, masks, goals, targets, met=None):
    """(palette [J, 16] float64 or None, weights [T] float64 or None)."""
    glob, w = layered_globals(desc, layers, masks, met)
    return palette_of(desc, model_globals_ik(desc, layers, masks, goals, targets, met, glob)), w


# ---------------------------------------------------------------------------------------------------------------- goals and targets
def depths(parents):
    d = np.zeros(len(parents), np.int64)
    for n, p in enumerate(parents):
        d[n] = 0 if p < 0 else d[p] + 1
    return d


def random_goals(desc, count_, rng, kinds="both"):
    """`count_` goals over the description's hierarchy: two-bone limbs root > mid > tip along random ancestor chains (nodes between them carried)
    and aims with random axes, in turn; chained and overlapping as the hierarchy makes them."""
    par = np.asarray(desc["parents"])
    dep = depths(par)
    deep = np.flatnonzero(dep >= 2)
    goals = []
    for k in range(count_):
        two = kinds == "two_bone" or (kinds == "both" and k % 2 == 0)
        if two and deep.size:
            tip = int(rng.choice(deep))
            chain = [tip]
            while par[chain[-1]] >= 0:
                chain.append(int(par[chain[-1]]))      # tip, its parent, ... , a root
            i = int(rng.integers(1, len(chain) - 1))
            j = int(rng.integers(i + 1, len(chain)))
            goals.append(TB(chain[j], chain[i], tip))
        else:
            axis = rng.standard_normal(3)
            goals.append(AIM(int(rng.integers(0, len(par))), tuple(float(x) for x in (axis / np.linalg.norm(axis)).astype(F))))
    return goals


def random_targets(desc, glob, goals, rng, reach="mixed"):
    """float32 [G, 8] for `goals` on the layered globals `glob`, drawn goal by goal on the model's own result of the goals before it, so that no
    decision of the model lies near its threshold: a two-bone target at a fraction of the limb's reach (inside: 0.35 .. 0.9; "beyond": 1.2 .. 1.6,
    in turn under reach="mixed"; reach="edge": the float32 value nearest to the reach, where sin(angle at A) ~ sqrt(reach - d) has no derivative, so no
    later goal is stacked on such a limb: the tests give it a case of its own) in a direction at least 0.2 rad off the limb's root bone and (with a pole, every second
    goal) off the pole; an aim target whose direction lies between 0.15 rad and 2.8 rad from the axis; weights 1, 0.5 and random in turn."""
    par = desc["parents"]
    rows = np.zeros((len(goals), 8), F)
    limbs = 0
    for k, g in enumerate(goals):
        w = (1.0, 0.5, float(F(rng.uniform(0.2, 0.95))))[k % 3]
        if isinstance(g, AIM):
            G = glob[g.node]
            v = unit(G[0, :3] * g.axis[0] + G[1, :3] * g.axis[1] + G[2, :3] * g.axis[2])
            while True:
                dr = unit(rng.standard_normal(3))
                if np.cos(2.8) < dr @ v < np.cos(0.15):
                    break
            rows[k] = np.concatenate([G[3, :3] + rng.uniform(0.5, 2.0) * dr, [w], np.zeros(4)]).astype(F)
        else:
            A, B, C = (glob[i][3, :3] for i in g)
            lab, lcb = np.linalg.norm(B - A), np.linalg.norm(C - B)
            lo, hi = abs(lab - lcb), lab + lcb
            kind = ("inside", "beyond", "inside", "inside")[limbs % 4] if reach == "mixed" else reach      # ("edge": asked for by name, a limb of its own)
            pole = limbs % 3 == 1
            limbs += 1
            if kind == "edge":
                w = 1.0      # (an edge target is met at full weight: the effective target of a partial weight lies elsewhere)
            while True:      # drawn again until the EFFECTIVE target (Te of the contract) is clear of every threshold
                dr, P = unit(rng.standard_normal(3)), A + rng.standard_normal(3)
                frac = {"inside": rng.uniform(0.35, 0.9), "edge": 1.0, "beyond": rng.uniform(1.2, 1.6)}[kind]
                T = (A + frac * hi * dr).astype(F).astype(D)
                Te = T if w == 1.0 else C + w * (T - C)
                d = np.linalg.norm(Te - A)
                if d < 0.05 * hi:
                    continue
                de = (Te - A) / d
                off = [np.linalg.norm(np.cross(de, unit(B - A)))] + ([np.linalg.norm(np.cross(de, unit(P - A)))] if pole else [])
                clear = kind == "edge" or (min(abs(d - lo), abs(d - hi)) > 0.02 * hi and d > lo)      # (never folded short of |lab - lcb|: see the degenerate cases)
                if min(off) > np.sin(0.2) and clear:
                    break
            rows[k] = np.concatenate([T, [w], P if pole else np.zeros(3), [1.0 if pole else 0.0]]).astype(F)
        glob = apply_goal(par, glob, g, rows[k])
    return rows
