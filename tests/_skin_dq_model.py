"""What the dual-quaternion skinning tests share (include/frt.h: frt_scene_set_mesh_skin_ex, FRT_SKIN_DUAL_QUATERNION; DESIGN.md section 11,
"Dual-quaternion skinning"): a float64 numpy model of the contract, restated here and not a call into the library, which records every decision it
takes with the margin it was taken by (the pivot slot, each sigma, the Shepperd branch), and generators of palettes, skins and the test meshes."""
import numpy as np

F, D = np.float32, np.float64
THIRD = D(F(1.0) / F(3.0))      # the contract's constant: 1/3 rounded to float32
BRANCHES = ("t", "R00", "R11", "R22")


def _branch_quat(R, b):
    """The unnormalised quaternion (x, y, z, w) of branch b; R[r, c] is row r, column c."""
    if b == 0:
        return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + ((R[0, 0] + R[1, 1]) + R[2, 2])], D)
    if b == 1:
        return np.array([((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]], D)
    if b == 2:
        return np.array([R[0, 1] + R[1, 0], ((1.0 + R[1, 1]) - R[0, 0]) - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]], D)
    return np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], ((1.0 + R[2, 2]) - R[0, 0]) - R[1, 1], R[1, 0] - R[0, 1]], D)


def joint_dq(mat):
    """One joint of the contract in float64: {"s", "qr", "qd", "branch", "branch_margin", "runner_up", "runner_up_gap"}. branch_margin: by how much the
    greatest of (t, R00, R11, R22) beat the second; runner_up_gap: max |qr - qr of the second branch| with the signs aligned (both are the same
    rotation: the choice is one of conditioning, and near a tie either is as good)."""
    m = np.asarray(mat, D).reshape(16)
    with np.errstate(all="ignore"):
        cols = np.stack([m[0:3], m[4:7], m[8:11]])                 # cols[c, r]
        n = (cols[:, 0] * cols[:, 0] + cols[:, 1] * cols[:, 1]) + cols[:, 2] * cols[:, 2]
        s = ((np.sqrt(n[0]) + np.sqrt(n[1])) + np.sqrt(n[2])) * THIRD
        R = (cols * (1.0 / np.sqrt(n))[:, None]).T                 # R[r, c]
        cand = np.array([(R[0, 0] + R[1, 1]) + R[2, 2], R[0, 0], R[1, 1], R[2, 2]], D)
        order = sorted(range(4), key=lambda k: (-cand[k], k)) if np.isfinite(cand).all() else [3, 2, 1, 0]
        b, b2 = order[0], order[1]
        q = _branch_quat(R, b)
        qr = q * (1.0 / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
        q2 = _branch_quat(R, b2)
        q2 = q2 / np.sqrt(q2 @ q2)
        if q2 @ qr < 0:
            q2 = -q2
        tx, ty, tz = m[12], m[13], m[14]
        x, y, z, w = qr
        qd = np.array([0.5 * ((tx * w + ty * z) - tz * y), 0.5 * ((ty * w + tz * x) - tx * z), 0.5 * ((tz * w + tx * y) - ty * x),
                       -0.5 * ((tx * x + ty * y) + tz * z)], D)
    return {"s": s, "qr": qr, "qd": qd, "branch": b, "branch_margin": float(cand[b] - cand[b2]), "runner_up": b2,
            "runner_up_gap": float(np.max(np.abs(q2 - qr)))}


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], D)


def skin_dq_model(positions, joints, weights, mats):
    """(out [n, 4] float64, decisions): the contract per vertex. decisions: "pivot" [n], "pivot_margin" [n] (the pivot's weight minus the greatest
    other weight: 0 for a tie, which the first-of-equals rule settles on the weights' own bits), "sigma" [n, 4], "sigma_margin" [n, 4] (|dot4| of
    each slot's qr with the pivot's), "joints": joint_dq of every joint of the palette."""
    p = np.asarray(positions, D)
    j, w = np.asarray(joints), np.asarray(weights, F).astype(D)
    jd = [joint_dq(m) for m in np.asarray(mats, D).reshape(-1, 16)]
    n = len(p)
    out = p.copy()
    dec = {"pivot": np.zeros(n, int), "pivot_margin": np.zeros(n), "sigma": np.ones((n, 4)), "sigma_margin": np.zeros((n, 4)), "joints": jd}
    with np.errstate(all="ignore"):
        for v in range(n):
            pi = 0
            for k in range(1, 4):
                if w[v, k] > w[v, pi]:
                    pi = k
            dec["pivot"][v] = pi
            dec["pivot_margin"][v] = w[v, pi] - max(w[v, k] for k in range(4) if k != pi)
            qs = [jd[j[v, k]] for k in range(4)]
            pr = qs[pi]["qr"]
            br, bd, sb = np.zeros(4, D), np.zeros(4, D), D(0)
            for k in range(4):
                a, b = qs[k]["qr"], pr
                dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
                sg = -1.0 if dot < 0 else 1.0
                dec["sigma"][v, k], dec["sigma_margin"][v, k] = sg, abs(dot)
                br = br + w[v, k] * (sg * qs[k]["qr"]) if k else w[v, 0] * (sg * qs[0]["qr"])
                bd = bd + w[v, k] * (sg * qs[k]["qd"]) if k else w[v, 0] * (sg * qs[0]["qd"])
                sb = sb + w[v, k] * qs[k]["s"] if k else w[v, 0] * qs[0]["s"]
            inv = 1.0 / np.sqrt(((br[0] * br[0] + br[1] * br[1]) + br[2] * br[2]) + br[3] * br[3])
            r, d = br * inv, bd * inv
            u, x = r[:3], sb * p[v, :3]
            rot = x + 2.0 * _cross(u, _cross(u, x) + r[3] * x)
            tr = 2.0 * ((r[3] * d[:3] - d[3] * u) + _cross(u, d[:3]))
            out[v, :3] = rot + tr
    return out, dec


def rotation(axis, angle):
    """[3, 3] float64, R[r, c]: Rodrigues."""
    a = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], D)
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def trs(R=None, t=(0.0, 0.0, 0.0), s=1.0):
    """One column-major 4x4 as [16] float32: T(t) * R * S(s)."""
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) if R is None else np.asarray(R, D)) * s
    m[:3, 3] = t
    return np.ascontiguousarray(m.T.reshape(16), F)


def random_palette(rng, njoints, scale=(1.0, 1.0), spread=1.0, max_angle=np.pi):
    """[njoints, 16] float32: a random rotation (any axis, an angle up to max_angle) times a uniform scale drawn from `scale`, a translation of `spread`."""
    out = np.zeros((njoints, 16), F)
    for k in range(njoints):
        out[k] = trs(rotation(rng.standard_normal(3), rng.uniform(-max_angle, max_angle)), spread * rng.standard_normal(3), rng.uniform(*scale))
    out[:, 15] = 1.0
    return out


def clear_skin(rng, n, mats, weights, sigma_clear=0.05, tries=200):
    """joints [n, 4] uint16 for the given weights such that the MODEL's sigma decisions all lie `sigma_clear` from zero: every vertex draws its four
    joints until its own dots with its pivot do. No vertex is dropped: a draw that fails `tries` times raises."""
    jd = [joint_dq(m)["qr"] for m in np.asarray(mats, D).reshape(-1, 16)]
    J = len(jd)
    out = np.zeros((n, 4), np.uint16)
    for v in range(n):
        pi = int(np.argmax(weights[v]))      # (numpy's argmax is the first of equals too)
        for _ in range(tries):
            c = rng.integers(0, J, 4)
            if all(abs(jd[c[k]] @ jd[c[pi]]) > sigma_clear for k in range(4)):
                out[v] = c
                break
        else:
            raise AssertionError("no clear draw")
    return out


def random_weights(rng, n):
    """[n, 4] float32: rows that sum to 1 up to rounding, every fifth with a zero, every seventh with two, every third unnormalised (sums 0.4 .. 1.6)."""
    w = rng.random((n, 4)).astype(F) + F(0.05)
    w[::5, 3] = 0.0
    w[::7, 1] = 0.0
    w = (w / w.sum(axis=1, keepdims=True)).astype(F)
    w[::3] *= rng.uniform(0.4, 1.6, (len(w[::3]), 1)).astype(F)
    return w


def ring_mesh(frt, n, radius=0.5, height=0.25, turns=1):
    """n vertices on a cylinder about the y axis, triangles (v, v + 1, v + 2) mod n: under an identity instance, triangle v's first world vertex IS
    vertex v's object-space position, so a host scene's "tris" rows give the posed positions back exactly."""
    a = np.linspace(0.0, 2.0 * np.pi * turns, n, endpoint=False)
    pos = np.stack([radius * np.cos(a), height * np.sin(3.0 * a), radius * np.sin(a), np.ones(n)], axis=1).astype(F)
    return mesh_of(frt, pos)


def mesh_of(frt, pos):
    pos = np.ascontiguousarray(pos, F)
    n = len(pos)
    att = np.zeros((n, 8), F)
    att[:, 0:2] = frt.geometry.encode_octahedral_normal([0.0, 1.0, 0.0])
    att[:, 4:8] = (1.0, 0.0, 0.0, 1.0)
    idx = np.array([[v, (v + 1) % n, (v + 2) % n] for v in range(n)], np.uint32).reshape(-1)
    return frt.geometry.Geometry(pos, att, idx)


def scene_of(frt, meshes):
    """A built scene with one identity instance per mesh, in mesh order, and one light no instance carries."""
    b = frt.SceneBuilder()
    for g in meshes:
        b.add_mesh(g)
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    for k in range(len(meshes)):
        b.add_instance(k, grey, np.eye(4, dtype=F).reshape(16))
    l = frt.Light()
    l.position[:] = (0.0, 1.5, 0.5); l.type_ = 0
    l.u[:] = (0.5, 0.0, 0.0); l.v[:] = (0.0, 0.0, 0.5); l.area = 1.0
    l.emission[:] = (1.0, 1.0, 1.0, 10.0)
    b.add_light(l)
    return b.build()


def posed_positions(fs, meshes, k):
    """The object-space xyz of mesh k of scene_of(meshes), read back from the world triangles (see ring_mesh)."""
    first = sum(len(g.positions) for g in meshes[:k])
    return fs.get("tris")[first:first + len(meshes[k].positions), 0:3].copy()
