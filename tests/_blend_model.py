"""What the blend tests share (include/frt.h: frt_rig_evaluate_blend; DESIGN.md section 11, "Blending clips"): a float64 restatement of the blend
contract over tests/_anim_model.py's sampling, matrices and products, and synthetic rigs whose EVERY clip has channels (make_rig's second clip has
none). A sample is (clip index, t, weight); a rig description is the dict of keyword arguments frt.Rig takes."""
import numpy as np
from _anim_model import F, D, WIDTH, INTERPS, sample, slerp, trs_matrix, mat_mul, make_rig, make_channel, unit_quats


# ---------------------------------------------------------------------------------------------------------------- the float64 model
def _rest(desc, n):
    tr = np.asarray(desc.get("translations") if desc.get("translations") is not None else np.zeros((n, 3)), F).astype(D)
    ro = np.asarray(desc.get("rotations") if desc.get("rotations") is not None else np.tile([0, 0, 0, 1], (n, 1)), F).astype(D)
    sc = np.asarray(desc.get("scales") if desc.get("scales") is not None else np.ones((n, 3)), F).astype(D)
    return {"translation": tr, "rotation": ro, "scale": sc}


def blend_steps(samples):
    """[(index into samples, a)] of the contract: the samples of weight 0 left out, a None for the first positive one, then w / W with W the
    sum of the weights so far (float32 weights, the sums and the quotient in float64)."""
    steps, W = [], None
    for i, (_, _, w) in enumerate(samples):
        w = D(F(w))
        if not w > 0.0:
            continue
        if W is None:
            steps.append((i, None)); W = w
        else:
            W = W + w
            steps.append((i, w / W))
    assert steps, "no positive weight"
    return steps


def model_evaluate_blend(desc, samples, met=None):
    """(palette [J, 16] float64 or None, weights [T] float64 or None) of the blend `samples`. met: a dict whose "min_abs_d" takes the smallest
    |dot product| a blend's slerp saw (the sign decision d < 0 is far from its threshold when that is large)."""
    par = np.asarray(desc["parents"])
    n = len(par)
    rest = _rest(desc, n)
    mats = desc.get("matrices") or {}
    steps = blend_steps(samples)
    by = {}
    for i, _ in steps:
        c = samples[i][0]
        if c not in by:
            by[c] = {(ch["node"], ch["path"]): ch for ch in desc["clips"][c][1] if ch["path"] != "weights"}

    def pose(i, node):
        c, t, _ = samples[i]
        return [sample(by[c][(node, p)], t, WIDTH[p], p == "rotation") if (node, p) in by[c] else rest[p][node] for p in ("translation", "rotation", "scale")]

    glob = [None] * n
    for node in range(n):
        if node in mats:
            local = np.asarray(mats[node], F).astype(D).reshape(4, 4)
        else:
            T = R = S = None
            for i, a in steps:
                t_s, r_s, s_s = pose(i, node)
                if a is None:
                    T, R, S = t_s, r_s, s_s
                    continue
                if met is not None:
                    met["min_abs_d"] = min(met.get("min_abs_d", 1.0), abs(float(np.dot(R, r_s))))
                T, S, R = T * (1.0 - a) + t_s * a, S * (1.0 - a) + s_s * a, slerp(R, r_s, a)
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
        for i, a in steps:
            c, t, _ = samples[i]
            wc = [ch for ch in desc["clips"][c][1] if ch["path"] == "weights"]
            w_s = sample(wc[0], t, nt) if wc else default
            w = w_s if a is None else w * (1.0 - a) + w_s * a
    return pal, w


# ---------------------------------------------------------------------------------------------------------------- synthetic rigs
def _quat_mul(a, b):
    x, y, z, w = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    X, Y, Z, W = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w * X + x * W + y * Z - z * Y, w * Y - x * Z + y * W + z * X, w * Z + x * Y - y * X + z * W, w * W - x * X - y * Y - z * Z], -1)


def near(rng, q, rows, spread):
    """`rows` unit quaternions, each `q` turned by at most `spread` radians about a random axis."""
    axis = rng.standard_normal((rows, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(0.0, spread, (rows, 1))
    dq = np.concatenate([np.sin(half) * axis, np.cos(half)], 1)
    out = _quat_mul(np.asarray(q, D)[None, :], dq)
    return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(F)


def make_blend_rig(shape, nclips=3, seed=0, joints="all", num_targets=3, keys=(1, 2, 5, 33), spread=0.5):
    """make_rig's topology, rest values, joints and matrix node, with `nclips` clips "c0", "c1", ... EVERY one of which has channels: translation,
    rotation and scale channels on about half the nodes each, drawn per clip (so two clips animate different, overlapping sets of limbs), every
    interpolation and key count in turn, and (with targets) a weights channel in every clip but the last, which takes the defaults.
    spread: every rotation key lies within that many radians of its node's rest rotation and the cubic tangents are small, so no two rotations a
    blend meets are far apart; None: fully random rotations, where the short way round does flip signs."""
    desc = make_rig(shape, seed=seed, joints=joints, num_targets=num_targets, keys=keys)
    rng = np.random.default_rng(sum(map(ord, shape)) + 7919 * seed + 104729)
    n = len(desc["parents"])
    clips, k = [], 0
    for c in range(nclips):
        channels = []
        for node in range(n):
            if node in desc.get("matrices", {}):
                continue
            for path in ("translation", "rotation", "scale"):
                if n <= 2 or rng.random() < 0.5:
                    ch = make_channel(rng, node, path, INTERPS[k % 3], keys[(k // 3) % len(keys)], t0=0.25 + 0.1 * c)
                    if path == "rotation" and spread is not None:
                        v = ch["values"]
                        if ch["interpolation"] == "CUBICSPLINE":
                            v[:, 1] = near(rng, desc["rotations"][node], len(v), spread)
                            v[:, 0::2] = F(0.02) * v[:, 0::2]
                        else:
                            ch["values"] = near(rng, desc["rotations"][node], len(v), spread)
                    channels.append(ch)
                    k += 1
        if not channels:      # (a tiny rig whose draw left a clip empty)
            channels.append(make_channel(rng, 0, "translation", "LINEAR", 2))
        if num_targets and (c + 1 < nclips or nclips == 1):
            channels.append(make_channel(rng, 0, "weights", INTERPS[c % 3], keys[-1], width=num_targets))
        clips.append((f"c{c}", channels))
    desc["clips"] = clips
    return desc


def clip_times(desc, clip, count, rng):
    """`count` float32 times for clip `clip`: before its first key, at key times, between keys, in turn."""
    keys = np.concatenate([c["times"] for c in desc["clips"][clip][1]])
    lo, hi = float(keys.min()), float(keys.max())
    out = []
    for i in range(count):
        kind = i % 3
        out.append(lo - 1.0 if kind == 0 and i < 3 else float(rng.choice(keys)) if kind != 2 else float(rng.uniform(lo, hi + 0.1)))
    return F(out)


def random_blends(desc, ns, count, seed=0, zero_at=None):
    """`count` blends of `ns` samples over the clips of `desc`: unequal, unnormalised weights in [0.1, 3], times before, at and between keys.
    zero_at: an index whose weight is 0 (negative: from the end)."""
    rng = np.random.default_rng(seed + 31 * ns)
    nclips = len(desc["clips"])
    out = []
    for b in range(count):
        clips = [(b + i) % nclips if i < nclips else int(rng.integers(0, nclips)) for i in range(ns)]
        rows = []
        for i, c in enumerate(clips):
            t = clip_times(desc, c, 3, rng)[(b + i) % 3]
            rows.append((c, float(t), float(F(rng.uniform(0.1, 3.0)))))
        if zero_at is not None and ns > 1:
            z = zero_at % ns
            rows[z] = (rows[z][0], rows[z][1], 0.0)
        out.append(rows)
    return out
