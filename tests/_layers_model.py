"""What the layer tests share (include/frt.h: frt_rig_evaluate_layers; DESIGN.md section 11, "Layering clips"): a float64 restatement of the layer
contract over tests/_anim_model.py's sampling, matrices and products, in the style of tests/_blend_model.py, and random layer stacks over
make_blend_rig's rigs. A model layer is an L(clip index, t, weight, mask index or None, mode, (reference clip, t) or None, morph); masks are
float32 [nmasks, nnodes] in the description's node order."""
from collections import namedtuple
import numpy as np
from _anim_model import F, D, WIDTH, sample, slerp, trs_matrix, mat_mul
from _blend_model import _rest, clip_times

L = namedtuple("L", "clip t weight mask mode reference morph", defaults=(1.0, None, "blend", None, True))
MODES = ("blend", "override", "additive")
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0], D)


def to_layers(frt, rows):
    """frt.Layer objects of model layers."""
    return [frt.Layer(r.clip, r.t, r.weight, mask=r.mask, mode=r.mode, reference=r.reference, morph=r.morph) for r in rows]


def qmul(a, b):
    x, y, z, w = a
    X, Y, Z, W = b
    return np.array([w * X + x * W + y * Z - z * Y, w * Y - x * Z + y * W + z * X, w * Z + x * Y - y * X + z * W, w * W - x * X - y * Y - z * Z], D)


def _note(met, q0, q1):
    """The two decisions of a slerp: the sign of the dot product and d > 0.9995."""
    if met is not None:
        d = abs(float(np.dot(q0, q1)))
        met["min_abs_d"] = min(met.get("min_abs_d", 1.0), d)
        met["min_gap"] = min(met.get("min_gap", 1.0), abs(d - float(D(F(0.9995)))))


def threshold_branch_gap(steps=1001):
    """The largest difference, in a component of a unit quaternion, between the two branches of the contract's slerp for two rotations exactly at
    its threshold d = 0.9995, over u in [0, 1], in float64: what a d > 0.9995 decision that falls differently in float32 and float64 can cost."""
    d = float(D(F(0.9995)))
    th = np.arccos(d)
    q0, q1 = IDENTITY, np.array([np.sin(th), 0.0, 0.0, np.cos(th)], D)
    worst = 0.0
    for u in np.linspace(0.0, 1.0, steps):
        mix = q0 * (1.0 - u) + q1 * u
        mix = mix / np.sqrt(np.dot(mix, mix))
        sine = q0 * (np.sin((1.0 - u) * th) / np.sin(th)) + q1 * (np.sin(u * th) / np.sin(th))
        worst = max(worst, float(np.abs(mix - sine).max()))
    return worst


def model_evaluate_layers(desc, layers, masks=None, met=None):
    """(palette [J, 16] float64 or None, weights [T] float64 or None) of the stack `layers` under `masks`. met: a dict whose "min_abs_d" takes the
    smallest |dot product| a slerp of the fold saw and "min_gap" the smallest distance of one from 0.9995."""
    par = np.asarray(desc["parents"])
    n = len(par)
    rest = _rest(desc, n)
    mats = desc.get("matrices") or {}
    masks = None if masks is None else np.asarray(masks, F).astype(D).reshape(-1, n)
    base = layers[0]
    assert base.mode == "blend" and base.mask is None and F(base.weight) > 0
    by = {}

    def channels(c):
        if c not in by:
            by[c] = {(ch["node"], ch["path"]): ch for ch in desc["clips"][c][1] if ch["path"] != "weights"}
        return by[c]

    def pose(c, t, node):
        ch = channels(c)
        return [sample(ch[(node, p)], t, WIDTH[p], p == "rotation") if (node, p) in ch else rest[p][node] for p in ("translation", "rotation", "scale")]

    glob = [None] * n
    for node in range(n):
        if node in mats:
            local = np.asarray(mats[node], F).astype(D).reshape(4, 4)
        else:
            T, R, S = pose(base.clip, base.t, node)
            W = D(F(base.weight))
            for l in layers[1:]:
                e = D(F(l.weight)) * (1.0 if l.mask is None else masks[l.mask][node])
                if not e > 0.0:
                    continue
                Xt, Xq, Xs = pose(l.clip, l.t, node)
                if l.mode == "additive":
                    Yt, Yq, Ys = pose(l.reference[0], l.reference[1], node)
                    T, S = T + e * (Xt - Yt), S + e * (Xs - Ys)
                    dq = qmul(np.array([-Yq[0], -Yq[1], -Yq[2], Yq[3]], D), Xq)
                    _note(met, IDENTITY, dq)
                    R = qmul(R, slerp(IDENTITY, dq, e))
                    continue
                if l.mode == "blend":
                    W = W + e
                    a = e / W
                else:
                    assert l.mode == "override"
                    a = e
                    if a >= 1.0:
                        T, R, S = Xt, Xq, Xs
                        continue
                _note(met, R, Xq)
                T, S, R = T * (1.0 - a) + Xt * a, S * (1.0 - a) + Xs * a, slerp(R, Xq, a)
            local = trs_matrix(T, R, S)
        glob[node] = local if par[node] < 0 else mat_mul(glob[par[node]], local)
    joints = np.asarray(desc.get("joint_nodes", ()), np.int64)
    pal = None
    if joints.size:
        ib = desc.get("inverse_bind")
        ib = np.tile(np.eye(4).reshape(16), (joints.size, 1)) if ib is None else np.asarray(ib, F).astype(D).reshape(-1, 16)
        pal = np.stack([mat_mul(glob[j], ib[k].reshape(4, 4)).reshape(16) for k, j in enumerate(joints)])
    nt = int(desc.get("num_targets", 0))
    w = None
    if nt:
        default = np.asarray(desc.get("default_weights") if desc.get("default_weights") is not None else np.zeros(nt), F).astype(D)

        def morph(c, t):
            wc = [ch for ch in desc["clips"][c][1] if ch["path"] == "weights"]
            return sample(wc[0], t, nt) if wc else default

        w, W = morph(base.clip, base.t), D(F(base.weight))
        for l in layers[1:]:
            e = D(F(l.weight))
            if not l.morph or not e > 0.0:
                continue
            x = morph(l.clip, l.t)
            if l.mode == "additive":
                w = w + e * (x - morph(*l.reference))
            elif l.mode == "blend":
                W = W + e
                w = w * (1.0 - e / W) + x * (e / W)
            else:
                w = x if e >= 1.0 else w * (1.0 - e) + x * e
    return pal, w


# ---------------------------------------------------------------------------------------------------------------- random stacks
def random_masks(desc, nmasks, seed=0, kind="fractional"):
    """[nmasks, nnodes] float32: "fractional" values drawn from [0, 1] with about a quarter exactly 0 and a quarter exactly 1; "binary" 0 / 1."""
    rng = np.random.default_rng(seed + 977)
    n = len(desc["parents"])
    m = rng.uniform(0.0, 1.0, (nmasks, n)).astype(F)
    pick = rng.random((nmasks, n))
    if kind == "binary":
        return (pick < 0.5).astype(F)
    m[pick < 0.25] = 0.0
    m[pick > 0.75] = 1.0
    return m


def random_stacks(desc, nl, count, mode, nmasks=0, seed=0):
    """`count` stacks of `nl` layers over the clips of `desc`: layer 0 the base, every later layer of mode `mode` ("mixed": the three in turn),
    unequal weights (blend in [0.1, 3], override in [0.1, 1] with an exact 1 now and then, additive in [0.1, 1.5]), times before, at and between
    keys, every second layer without its morph share, and with nmasks > 0 a mask on two layers out of three."""
    rng = np.random.default_rng(seed + 31 * nl + 7 * MODES.index(mode) if mode in MODES else seed + 31 * nl + 29)
    nclips = len(desc["clips"])
    out = []
    for b in range(count):
        rows = []
        for i in range(nl):
            c = (b + i) % nclips if i < nclips else int(rng.integers(0, nclips))
            t = float(clip_times(desc, c, 3, rng)[(b + i) % 3])
            if i == 0:
                rows.append(L(c, t, float(F(rng.uniform(0.1, 3.0)))))
                continue
            m = MODES[(b + i) % 3] if mode == "mixed" else mode
            hi = {"blend": 3.0, "override": 1.0, "additive": 1.5}[m]
            w = float(F(rng.uniform(0.1, hi)))
            if m == "override" and (b + i) % 4 == 0:
                w = 1.0
            mask = int(rng.integers(0, nmasks)) if nmasks and (b + i) % 3 != 0 else None
            ref = None
            if m == "additive":
                rc = int(rng.integers(0, nclips))
                ref = (rc, float(clip_times(desc, rc, 3, rng)[i % 3]))
            rows.append(L(c, t, w, mask, m, ref, (b + i) % 2 == 0))
        out.append(rows)
    return out


def splice(desc, a, b, nodes):
    """The node channels of a clip that is clip `b` on `nodes` and clip `a` elsewhere. No weights channel is copied: the caller adds the one it
    means."""
    nodes = set(int(x) for x in nodes)
    return [ch for ch in desc["clips"][a][1] if ch["path"] != "weights" and ch["node"] not in nodes] + \
           [ch for ch in desc["clips"][b][1] if ch["path"] != "weights" and ch["node"] in nodes]
