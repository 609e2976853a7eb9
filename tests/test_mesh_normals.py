"""Recomputed vertex normals on the host (include/frt.h: frt_scene_set_mesh_vertices_ex, FRT_DEFORM_RECOMPUTE_NORMALS; DESIGN.md section 11, "Recomputed
normals"): the specification against an independent float32 numpy model written here — the same expressions in the same order; numpy's f32 + - * /
sqrt are IEEE — bit for bit, through the existing call (the model's attributes given explicitly) and through a build from scratch."""
import numpy as np
import pytest
from test_instance_update import cornell_meshes, by_id, SELECTORS
from test_mesh_deform import deform, cornell_with, _decode_oct, assert_equals_fresh, PLANE, CUBE, SPHERE

EVERYTHING = SELECTORS + ("shade_tris", "attributes", "materials", "indices", "mesh_infos", "tri_slots", "quad_nodes", "pair_nodes")
F = np.float32
RECOMPUTE, DEVICE = 1, 2      # include/frt.h: FRT_DEFORM_RECOMPUTE_NORMALS, FRT_DEFORM_DEVICE


def _encode(n):
    """geometry.rs:56-76 in f32, operation by operation."""
    l1 = (np.abs(n[0]) + np.abs(n[1])) + np.abs(n[2])
    rx, ry = F(0.0), F(0.0)
    if l1 > 0:
        rx, ry = n[0] / l1, n[1] / l1
    if n[2] < 0:
        rx, ry = (F(1.0) - np.abs(ry)) * (F(1.0) if rx >= 0 else F(-1.0)), (F(1.0) - np.abs(rx)) * (F(1.0) if ry >= 0 else F(-1.0))
    return F(rx), F(ry)


def model_normals(positions, indices, attributes):
    """The attributes after a recomputation: per vertex s = ((0 + c_a) + c_b) + ... over its corners in ascending 3 j + corner, c_j = e1 x e2 of the
    corner's triangle; d = (sx sx + sy sy) + sz sz; no corner, d == 0 or d not finite keeps the record; else normal = encode(s * (1 / sqrt(d)))."""
    P = np.asarray(positions, F)[:, :3]
    idx = np.asarray(indices, np.int64)
    att = np.array(attributes, F)
    s = np.zeros((len(P), 3), F)
    seen = np.zeros(len(P), bool)
    with np.errstate(all="ignore"):
        for c, v in enumerate(idx):                       # ascending corner order is the summation order of every vertex
            i0, i1, i2 = idx[3 * (c // 3):3 * (c // 3) + 3]
            e1, e2 = P[i1] - P[i0], P[i2] - P[i0]
            cj = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
            s[v] = s[v] + cj
            seen[v] = True
        for v in range(len(P)):
            d = (s[v, 0] * s[v, 0] + s[v, 1] * s[v, 1]) + s[v, 2] * s[v, 2]
            if not seen[v] or not np.isfinite(d) or d == 0:
                continue
            r = F(1.0) / np.sqrt(d)
            assert r.dtype == F
            att[v, 0:2] = _encode(s[v] * r)
    return att


def _everything(s):
    return {w: s.get(w).tobytes() for w in EVERYTHING}


def _same(a, b, what):
    for w in EVERYTHING:
        assert a.get(w).tobytes() == b.get(w).tobytes(), f"{what}: {w}"


@pytest.fixture(scope="module")
def cases(frt):
    """Cornell Box mesh id -> (new positions, the model's attributes): the sphere (642 shared vertices, valence 5 and 6) and the cube (unshared corners)
    under test_mesh_deform.deform, the plane (4 vertices, valence 1 and 2) bent out of its plane."""
    base = cornell_meshes(frt)
    pos = {m: np.array(deform(frt, base[m], 0.3 * m).positions, F) for m in (SPHERE, CUBE)}
    p = np.array(base[PLANE].positions, F)
    p[:, 1] = F(0.2) * p[:, 0] * p[:, 2] + F(0.05) * p[:, 0]
    pos[PLANE] = p
    return base, {m: (pos[m], model_normals(pos[m], base[m].indices, base[m].attributes)) for m in pos}


@pytest.mark.parametrize("mesh", [SPHERE, PLANE, CUBE], ids=["sphere", "plane", "cube"])
def test_recomputed_normals_equal_the_numpy_model(frt, cases, mesh):
    base, new = cases
    pos, att = new[mesh]
    assert (att[:, 0:2] != np.asarray(base[mesh].attributes, F)[:, 0:2]).any()            # the model moved some normal
    assert np.array_equal(att[:, 2:8], np.asarray(base[mesh].attributes, F)[:, 2:8])      # ... and nothing else
    s = frt.scenes.create_cornell_box()
    s.set_mesh_vertices(mesh, pos, normals="recompute")
    want = frt.scenes.create_cornell_box().set_mesh_vertices(mesh, pos, att)              # the existing call, given the model's attributes
    _same(s, want, "recompute vs the model's attributes")
    meshes = list(base)
    meshes[mesh] = frt.geometry.Geometry(pos, att, base[mesh].indices)
    fresh = cornell_with(frt, meshes)
    assert_equals_fresh(s, fresh, "recompute vs a build from scratch:")
    mi = fresh.get("mesh_infos")[mesh]
    assert s.get("attributes")[mi[0]:mi[0] + len(att)].tobytes() == att.tobytes()


def test_valences_and_hard_edges(frt, cases):
    base, _ = cases
    val = {m: np.bincount(np.asarray(base[m].indices), minlength=len(base[m].positions)) for m in (SPHERE, PLANE, CUBE)}
    assert len(val[SPHERE]) == 642 and set(val[SPHERE]) == {5, 6} and sorted(val[PLANE]) == [1, 1, 2, 2] and set(val[CUBE]) <= {1, 2}
    # the undeformed cube: every corner is three vertices, one per face, and each gets its face's normal back (a smooth cube would round the edges)
    cube = base[CUBE]
    att = model_normals(cube.positions, cube.indices, cube.attributes)
    assert np.array_equal(att, np.asarray(cube.attributes, F))                           # (value equality: -0 == 0)
    s = frt.scenes.create_cornell_box()
    shade = s.get("shade_tris").copy()
    s.set_mesh_vertices(CUBE, cube.positions, normals="recompute")
    assert np.array_equal(s.get("shade_tris"), shade)
    # the undeformed sphere: recomputed normals point outwards, within the half-angle of a face (edges of about 8 degrees) of the analytic ones
    sph = base[SPHERE]
    got = model_normals(sph.positions, sph.indices, sph.attributes)
    cos = (_decode_oct(got[:, 0:2].astype(np.float64)) * _decode_oct(np.asarray(sph.attributes, np.float64)[:, 0:2])).sum(axis=1)
    assert cos.min() > np.cos(np.radians(4.0))


def _hand_made(frt):
    """Triangle A (0, 1, 2); (1, 2, 2) names vertex 2 twice; (3, 4, 5) has no area (collinear); vertex 6 is named by nothing; B (7, 8, 0) shares vertex 0."""
    pos = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0.25, 1], [2, 0, 0, 1], [3, 0, 0, 1], [4, 0, 0, 1], [5, 5, 5, 1], [0, -1, 0.5, 1], [-1, 0, 0.125, 1]], F)
    idx = np.array([0, 1, 2, 1, 2, 2, 3, 4, 5, 7, 8, 0], np.uint32)
    att = np.zeros((len(pos), 8), F)
    rng = np.random.default_rng(11)
    for v in range(len(pos)):
        n = rng.normal(size=3).astype(F)
        att[v, 0:2] = frt.geometry.encode_octahedral_normal(n / np.linalg.norm(n))
    att[:, 2:4] = rng.random((len(pos), 2), dtype=F)
    att[:, 4:8] = [1, 0, 0, 1]
    return frt.geometry.Geometry(pos, att, idx)


def _hand_scene(frt, g):
    b = frt.SceneBuilder()
    b.add_mesh(g)
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(0, mat, np.eye(4, dtype=F))
    b.add_instance(0, mat, np.diag(np.array([-2.0, 1.0, 1.0, 1.0], F)))      # mirrored
    return b.build()


def test_degenerate_corners_keep_their_attribute_words(frt):
    g = _hand_made(frt)
    pos = np.array(g.positions, F)
    pos[[0, 1, 2, 7, 8], 2] += F(0.125)
    want = model_normals(pos, g.indices, g.attributes)
    kept = [3, 4, 5, 6]
    assert want[kept].tobytes() == np.asarray(g.attributes, F)[kept].tobytes()
    assert (want[[0, 1, 2, 7, 8], 0:2] != np.asarray(g.attributes, F)[[0, 1, 2, 7, 8], 0:2]).any(axis=1).all()
    s = _hand_scene(frt, g)
    s.set_mesh_vertices(0, pos, normals="recompute")
    assert s.get("attributes").tobytes() == want.tobytes()
    _same(s, _hand_scene(frt, g).set_mesh_vertices(0, pos, want), "hand-made mesh")
    fresh = _hand_scene(frt, frt.geometry.Geometry(pos, want, g.indices))
    for w in ("tris", "shade_tris", "attributes", "instances_dev"):
        assert s.get(w).tobytes() == fresh.get(w).tobytes(), w
    assert by_id(s.get("tri_slots")).tobytes() == by_id(fresh.get("tri_slots")).tobytes()


def test_closure_and_given_attributes(frt, cases):
    base, new = cases
    pos, att = new[SPHERE]
    s = frt.scenes.create_cornell_box().set_mesh_vertices(SPHERE, pos, normals="recompute")
    mi = s.get("mesh_infos")[SPHERE]
    back = s.get("attributes")[mi[0]:mi[0] + len(pos)]
    _same(frt.scenes.create_cornell_box().set_mesh_vertices(SPHERE, pos, attributes=back), s, "closure")
    # attributes given: uv and tangent are the argument's, the normal is recomputed
    given = np.array(deform(frt, base[SPHERE], 1.7).attributes, F)
    given[:, 4:8] = [0.0, 1.0, 0.0, -1.0]
    s2 = frt.scenes.create_cornell_box().set_mesh_vertices(SPHERE, pos, given, normals="recompute")
    got = s2.get("attributes")[mi[0]:mi[0] + len(pos)]
    assert got[:, 2:8].tobytes() == given[:, 2:8].tobytes() and got[:, 0:2].tobytes() == att[:, 0:2].tobytes()
    mixed = given.copy(); mixed[:, 0:2] = att[:, 0:2]
    _same(s2, frt.scenes.create_cornell_box().set_mesh_vertices(SPHERE, pos, mixed), "given attributes")


def test_keep_is_the_existing_call(frt, cases):
    base, new = cases
    pos, att = new[SPHERE]
    n = len(pos)
    for a in (None, att):
        s = frt.scenes.create_cornell_box().set_mesh_vertices(SPHERE, pos, a, normals="keep")
        old, ex = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
        p = np.ascontiguousarray(pos); q = np.ascontiguousarray(a) if a is not None else None
        assert frt.lib().frt_scene_set_mesh_vertices(old._h, SPHERE, p.ctypes.data, q.ctypes.data if q is not None else None, n) == 0
        assert frt.lib().frt_scene_set_mesh_vertices_ex(ex._h, SPHERE, p.ctypes.data, q.ctypes.data if q is not None else None, n, 0) == 0
        _same(s, old, "keep vs frt_scene_set_mesh_vertices")
        _same(ex, old, "flags = 0 vs frt_scene_set_mesh_vertices")


def test_errors_change_nothing(frt, cases):
    _, new = cases
    pos, att = new[SPHERE]
    s = frt.scenes.create_cornell_box()
    before = _everything(s)
    p = np.ascontiguousarray(pos)
    for flags in (4, 1 | 4, 0x80000000, DEVICE, DEVICE | RECOMPUTE):                     # unknown bits; the device flag on a scene
        assert frt.lib().frt_scene_set_mesh_vertices_ex(s._h, SPHERE, p.ctypes.data, None, len(p), flags) == -1, flags
    bad = pos.copy(); bad[5, 0] = np.nan
    for args in ((SPHERE, bad, None), (99, pos, None), (SPHERE, pos[:-1], None), (SPHERE, pos, att[:-1])):
        with pytest.raises(frt.FrtError):
            s.set_mesh_vertices(*args, normals="recompute")
    with pytest.raises(frt.FrtError, match="normals must be"):
        s.set_mesh_vertices(SPHERE, pos, normals="smooth")
    assert _everything(s) == before
    b = frt.SceneBuilder()
    b.add_mesh(cases[0][PLANE])
    b.add_instance(0, 0xFFFFFFFF, np.eye(4, dtype=F))
    with pytest.raises(frt.FrtError, match="error -4"):
        b.set_mesh_vertices(0, new[PLANE][0], normals="recompute")                       # not built
