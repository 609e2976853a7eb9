"""What the animation tests share (include/frt.h: frt_rig_evaluate; DESIGN.md section 11, "Animation"): a float64 numpy restatement of the contract
(np.arccos, np.sin, matrix products in the stated association) and deterministic synthetic rigs. A rig description is the dict of keyword arguments
frt.Rig takes, so `frt.Rig(**desc)` builds what `model_evaluate(desc, clip, t)` models."""
import numpy as np

F = np.float32
D = np.float64
WIDTH = {"translation": 3, "rotation": 4, "scale": 3}


# ---------------------------------------------------------------------------------------------------------------- the float64 model
def find_key(times, t):
    """(k, between, u, dt) of the contract's sampling rule; times float32, t a float32 value."""
    times = np.asarray(times, F).astype(D)
    t = D(F(t))
    K = len(times)
    if t <= times[0]:
        return 0, False, 0.0, 0.0
    if t >= times[K - 1]:
        return K - 1, False, 0.0, 0.0
    k = int(np.searchsorted(times, t, side="right")) - 1
    if t == times[k]:
        return k, False, 0.0, 0.0
    dt = times[k + 1] - times[k]
    return k, True, (t - times[k]) / dt, dt


def slerp(q0, q1, u):
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    if d > D(F(0.9995)):
        q = q0 * (1.0 - u) + q1 * u
        return q / np.sqrt(np.dot(q, q))
    th = np.arccos(d)
    return q0 * (np.sin((1.0 - u) * th) / np.sin(th)) + q1 * (np.sin(u * th) / np.sin(th))


def sample(ch, t, width, rotation=False):
    v = np.asarray(ch["values"], F).astype(D)
    k, between, u, dt = find_key(ch["times"], t)
    interp = ch.get("interpolation", "LINEAR")
    if interp == "CUBICSPLINE":
        v = v.reshape(-1, 3, width)
        if not between:
            return v[k, 1]
        u2, u3 = u * u, u * u * u
        r = (2 * u3 - 3 * u2 + 1) * v[k, 1] + dt * (u3 - 2 * u2 + u) * v[k, 2] + (3 * u2 - 2 * u3) * v[k + 1, 1] + dt * (u3 - u2) * v[k + 1, 0]
        return r / np.sqrt(np.dot(r, r)) if rotation else r
    v = v.reshape(-1, width)
    if not between or interp == "STEP":
        return v[k]
    return slerp(v[k], v[k + 1], u) if rotation else v[k] * (1.0 - u) + v[k + 1] * u


def trs_matrix(t, q, s):
    """Column-major [c, r] T R S."""
    x, y, z, w = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)],
                  [2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)],
                  [2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)]], D)      # r[c] = column c
    m = np.zeros((4, 4), D)
    m[:3, :3] = r * np.asarray(s, D)[:, None]
    m[3, :3] = t
    m[3, 3] = 1.0
    return m


def mat_mul(a, b):
    """Column-major [c, r] product A B."""
    return (a.T @ b.T).T


def model_evaluate(desc, clip, t):
    """(palette [J, 16] float64 or None, weights [T] float64 or None)."""
    par = np.asarray(desc["parents"])
    n = len(par)
    tr = np.asarray(desc.get("translations") if desc.get("translations") is not None else np.zeros((n, 3)), F).astype(D)
    ro = np.asarray(desc.get("rotations") if desc.get("rotations") is not None else np.tile([0, 0, 0, 1], (n, 1)), F).astype(D)
    sc = np.asarray(desc.get("scales") if desc.get("scales") is not None else np.ones((n, 3)), F).astype(D)
    mats = desc.get("matrices") or {}
    channels = desc["clips"][clip][1] if desc.get("clips") else []
    by = {(c["node"], c["path"]): c for c in channels if c["path"] != "weights"}
    glob = [None] * n
    for i in range(n):
        if i in mats:
            local = np.asarray(mats[i], F).astype(D).reshape(4, 4)
        else:
            a = [sample(by[(i, p)], t, WIDTH[p], p == "rotation") if (i, p) in by else rest[i] for p, rest in (("translation", tr), ("rotation", ro), ("scale", sc))]
            local = trs_matrix(*a)
        glob[i] = local if par[i] < 0 else mat_mul(glob[par[i]], local)
    joints = np.asarray(desc.get("joint_nodes", ()), np.int64)
    pal = None
    if joints.size:
        ib = desc.get("inverse_bind")
        ib = np.tile(np.eye(4).reshape(16), (joints.size, 1)) if ib is None else np.asarray(ib, F).astype(D).reshape(-1, 16)
        pal = np.stack([mat_mul(glob[j], ib[k].reshape(4, 4)).reshape(16) for k, j in enumerate(joints)])
    nt = int(desc.get("num_targets", 0))
    w = None
    if nt:
        wc = [c for c in channels if c["path"] == "weights"]
        if wc:
            w = sample(wc[0], t, nt)
        else:
            w = np.asarray(desc.get("default_weights") if desc.get("default_weights") is not None else np.zeros(nt), F).astype(D)
    return pal, w


# ---------------------------------------------------------------------------------------------------------------- synthetic rigs
def parents_of(shape, rng):
    """chain<d>: a chain of d nodes; fan<k>: a root with k children (k nodes on one level); tree<n>: n nodes, each under a random earlier one."""
    kind, n = shape.rstrip("0123456789"), int(shape[len(shape.rstrip("0123456789")):])
    if kind == "chain":
        return np.arange(-1, n - 1, dtype=np.int32)
    if kind == "fan":
        return np.array([-1] + [0] * n, np.int32)
    assert kind == "tree"
    return np.array([-1] + [int(rng.integers(0, i)) for i in range(1, n)], np.int32)


def unit_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def make_channel(rng, node, path, interp, nkeys, width=None, t0=0.25):
    width = width or WIDTH[path]
    times = (t0 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.3, nkeys - 1))])).astype(F)
    rows = nkeys * (3 if interp == "CUBICSPLINE" else 1)
    if path == "rotation":
        v = unit_quats(rng, rows)
    elif path == "scale":
        v = rng.uniform(0.9, 1.1, (rows, width)).astype(F)
    else:
        v = (0.3 * rng.standard_normal((rows, width))).astype(F)
    if interp == "CUBICSPLINE":
        v = v.reshape(nkeys, 3, width)
        v[:, 0] = (0.5 * rng.standard_normal((nkeys, width))).astype(F)
        v[:, 2] = (0.5 * rng.standard_normal((nkeys, width))).astype(F)
    return {"node": int(node), "path": path, "interpolation": interp, "times": times, "values": v}


INTERPS = ("STEP", "LINEAR", "CUBICSPLINE")


def make_rig(shape, seed=0, joints="all", num_targets=3, keys=(1, 2, 5, 33), weights_interp="LINEAR"):
    """A random rig description. joints: "all" (every node, permuted), "subset" (a permuted strict subset) or "none" (a morph-only rig). One clip with
    translation, rotation and scale channels on about half the nodes each, every interpolation and every key count of `keys` in turn, and (with
    targets) a weights channel; a second clip without channels (the rest pose and the default weights)."""
    rng = np.random.default_rng(sum(map(ord, shape)) + 7919 * seed)
    par = parents_of(shape, rng)
    n = len(par)
    desc = {"parents": par, "translations": (0.3 * rng.standard_normal((n, 3))).astype(F), "rotations": unit_quats(rng, n),
            "scales": rng.uniform(0.95, 1.05, (n, 3)).astype(F), "num_targets": num_targets}
    if n > 3:      # one node given as a matrix (a leaf of the numbering: it has no channel below)
        m = np.eye(4, dtype=F)
        m[:3, :3] += (0.1 * rng.standard_normal((3, 3))).astype(F)
        m[3, :3] = (0.2 * rng.standard_normal(3)).astype(F)
        desc["matrices"] = {n - 2: m.reshape(16)}
    if joints != "none":
        order = rng.permutation(n)
        jn = order if joints == "all" else order[:max(1, n // 2)]
        ib = np.tile(np.eye(4, dtype=F).reshape(16), (len(jn), 1))
        ib[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (0.1 * rng.standard_normal((len(jn), 9))).astype(F)
        ib[:, 12:15] = (0.2 * rng.standard_normal((len(jn), 3))).astype(F)
        desc["joint_nodes"], desc["inverse_bind"] = jn.astype(np.uint32), ib
    channels, k = [], 0
    for node in range(n):
        if node in desc.get("matrices", {}):
            continue
        for path in ("translation", "rotation", "scale"):
            if n <= 2 or rng.random() < 0.5:
                channels.append(make_channel(rng, node, path, INTERPS[k % 3], keys[(k // 3) % len(keys)]))
                k += 1
    if num_targets:
        desc["default_weights"] = rng.uniform(0.0, 1.0, num_targets).astype(F)
        channels.append(make_channel(rng, 0, "weights", weights_interp, keys[-1], width=num_targets))
    desc["clips"] = [("move", channels), ("rest", [])]
    return desc


def sample_times(desc, count, seed=0):
    """`count` float32 times for clip 0: before the first key, after the last, at key times, and between keys."""
    rng = np.random.default_rng(seed + 17)
    keys = np.concatenate([c["times"] for c in desc["clips"][0][1]] or [np.zeros(1, F)])
    lo, hi = float(keys.min()), float(keys.max())
    fixed = [lo - 1.0, hi + 1.0, lo, hi] + [float(x) for x in rng.choice(keys, size=min(4, keys.size), replace=False)]
    return np.array(fixed[:count] + list(rng.uniform(lo - 0.1, hi + 0.1, max(0, count - len(fixed)))), F)
