"""Deforming a mesh of a built scene (include/frt.h: frt_scene_set_mesh_vertices; DESIGN.md section 11, "Deforming meshes"), on the host: the same
tree with its boxes refit; triangles, triangle slots, shading records and attributes equal, byte for byte, to a scene built from scratch with the
deformed meshes; instance records and lights untouched (a registered light follows its transform, not its mesh); errors change nothing; no stale
8-wide tree. One deterministic deformation is used everywhere: every comparison is against a fresh build from the same data."""
import numpy as np
import pytest
from test_instance_update import cornell_meshes, cornell_moves, move, by_id, check_boxes, SELECTORS, QUAD_LIGHT, SPHERE_LIGHT, CRYSTAL

PLANE, CUBE, SPHERE, CRYSTAL_MESH = 0, 1, 2, 3      # Cornell Box mesh ids (scenes.rs:9-14 order)
COMPARED = ("tris", "tri_instance", "shade_tris", "attributes", "instances", "instances_dev", "lights", "materials", "indices", "mesh_infos")
EVERYTHING = SELECTORS + ("shade_tris", "attributes", "materials", "indices", "mesh_infos")


def _decode_oct(e):
    n = np.stack([e[:, 0], e[:, 1], 1.0 - np.abs(e[:, 0]) - np.abs(e[:, 1])], axis=1)
    t = np.maximum(-n[:, 2], 0.0)
    n[:, 0] += np.where(n[:, 0] >= 0.0, -t, t)
    n[:, 1] += np.where(n[:, 1] >= 0.0, -t, t)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def deform(frt, g, phase=0.0):
    """p' = p * (1 + 0.15 sin(7 p.y + 3 p.x + phase)); normals perturbed, renormalised and encoded again; uvs shifted. Same topology."""
    pos = np.array(g.positions, np.float32)
    p = pos[:, :3].copy()
    pos[:, :3] = p * (np.float32(1.0) + np.float32(0.15) * np.sin(np.float32(7.0) * p[:, 1] + np.float32(3.0) * p[:, 0] + np.float32(phase)))[:, None]
    att = np.array(g.attributes, np.float32)
    n = _decode_oct(att[:, 0:2].astype(np.float64)) + 0.2 * np.stack([np.sin(5.0 * p[:, 0] + phase), np.cos(4.0 * p[:, 1]), np.sin(3.0 * p[:, 2] + 1.0)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    att[:, 0:2] = np.stack([frt.geometry.encode_octahedral_normal(v) for v in n.astype(np.float32)])
    att[:, 2:4] += np.float32(0.125)
    return frt.geometry.Geometry(pos, att, g.indices)


def cornell_with(frt, meshes, moves=None):
    """test_instance_update.cornell with the given meshes: the Cornell Box issued call by call, instance k at moves[k] where given."""
    moves = moves or {}
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    b = frt.SceneBuilder()
    for g in meshes:
        b.add_mesh(g)
    for k in range(6):
        b.add_material(frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()))
    for k, row in enumerate(inst):
        m = np.asarray(moves[k], np.float32).reshape(16) if k in moves else row[5:21].view(np.float32)
        if k == QUAD_LIGHT:
            b.register_quad_light(int(row[0]), m, (1.0, 1.0, 1.0), 10.0)
        elif k == SPHERE_LIGHT:
            b.register_sphere_light(int(row[0]), m, (0.02, 0.02, 0.9), 10.0)
        else:
            b.add_instance(int(row[0]), int(row[1]), m)
    return b.build()


def mesh_work(scene, mesh_id):
    """Triangles a deformation of the mesh rewrites: the summed triangle count of its instances."""
    inst = scene.get("instances")
    return int(inst[inst[:, 0] == mesh_id, 3].sum())


def _counts(s):
    """Node and slot counts of the binary, pair and quad trees (the 8-wide tree is made again from the refit binary tree and may fold differently)."""
    t = s.tree_stats()
    return (s.counts()["bvh2_nodes"], s.bvh_stats(), t["quad_nodes"], t["quad_stack_need"], t["quad_fold"], t["wide8_tri_slots"], len(s.get("tri_slots")))


def assert_equals_fresh(s, fresh, what=""):
    for w in COMPARED:
        assert s.get(w).tobytes() == fresh.get(w).tobytes(), f"{what} {w}"
    assert by_id(s.get("tri_slots")).tobytes() == by_id(fresh.get("tri_slots")).tobytes(), f"{what} tri_slots"


@pytest.fixture(scope="module")
def deformed(frt):
    """The Cornell Box meshes and their deformed forms (mesh id -> Geometry), made once."""
    base = cornell_meshes(frt)
    return base, {m: deform(frt, base[m], 0.3 * m) for m in (PLANE, SPHERE, CRYSTAL_MESH)}


def test_shade_tris_selector(frt):
    s = frt.scenes.create_cornell_box()
    rec = s.get("shade_tris")
    assert rec.shape == (s.counts()["tris"], 32)
    inst, ti = s.get("instances"), s.get("tri_instance")
    assert np.array_equal(rec[:, 25].view(np.uint32), inst[ti, 1])                   # the material id of the triangle's instance
    assert np.allclose(np.linalg.norm(rec[:, 0:3], axis=1), 1.0, atol=1e-6)          # decoded normals
    assert not rec[:, 26:32].any()
    att, idx, mi = s.get("attributes"), s.get("indices"), s.get("mesh_infos")
    k = int(inst[CRYSTAL, 2]) + 1                                                    # one triangle by hand: uvs of its corners in the .w lanes
    prim, mesh = 1, int(inst[CRYSTAL, 0])
    corner = [att[idx[mi[mesh, 1] + 3 * prim + c] + mi[mesh, 0]] for c in range(3)]
    assert rec[k, [3, 7]].tolist() == corner[0][2:4].tolist() and rec[k, [11, 15]].tolist() == corner[1][2:4].tolist()
    assert rec[k, [19, 23]].tolist() == corner[2][2:4].tolist() and rec[k, 24] == corner[0][7]
    assert rec[k, 12:15].tolist() == corner[0][4:7].tolist()


def test_deformed_cornell_matches_a_fresh_build(frt, deformed):
    """Successive calls: the sphere (used by the sphere light), the plane (the walls and the quad light), the crystal (mirrored by the moves)."""
    base, new = deformed
    moves = cornell_moves(frt)
    s = move(frt.scenes.create_cornell_box(), moves)
    orig = frt.scenes.create_cornell_box()
    stats = _counts(s)
    meshes = list(base)
    assert s.get("instances")[CRYSTAL, 4] == 1                                        # mirrored: flip
    assert mesh_work(s, PLANE) > 2                                                    # several instances share the plane
    for m in (SPHERE, PLANE, CRYSTAL_MESH):
        before = s.get("tris").copy()
        s.set_mesh_vertices(m, new[m].positions, new[m].attributes)
        meshes[m] = new[m]
        assert_equals_fresh(s, cornell_with(frt, meshes, moves), f"after mesh {m}:")
        inst = s.get("instances")
        changed = np.flatnonzero((s.get("tris") != before).any(axis=1))
        assert changed.size and set(s.get("tri_instance")[changed]) <= set(np.flatnonzero(inst[:, 0] == m))
        check_boxes(s)
    # the tree is the original one, refit; lights are derived from transforms and have not followed their meshes
    assert np.array_equal(s.get("bvh2_tri_index"), orig.get("bvh2_tri_index"))
    assert np.array_equal(s.get("bvh2_nodes")[:, [3, 7]], orig.get("bvh2_nodes")[:, [3, 7]])
    assert np.array_equal(s.get("quad_nodes")[:, 24:28].view(np.uint32), orig.get("quad_nodes")[:, 24:28].view(np.uint32))
    assert np.array_equal(s.get("pair_nodes")[:, 12:14].view(np.uint32), orig.get("pair_nodes")[:, 12:14].view(np.uint32))
    assert _counts(s) == stats == _counts(orig)
    assert s.get("lights").tobytes() == move(frt.scenes.create_cornell_box(), moves).get("lights").tobytes()


def test_positions_only_keeps_attributes_and_shading_records(frt, deformed):
    base, new = deformed
    s = frt.scenes.create_cornell_box()
    rec, att = s.get("shade_tris").tobytes(), s.get("attributes").tobytes()
    s.set_mesh_vertices(SPHERE, new[SPHERE].positions)
    assert s.get("shade_tris").tobytes() == rec and s.get("attributes").tobytes() == att
    meshes = list(base)
    meshes[SPHERE] = frt.geometry.Geometry(new[SPHERE].positions, base[SPHERE].attributes, base[SPHERE].indices)
    assert_equals_fresh(s, cornell_with(frt, meshes), "positions only:")
    check_boxes(s)


@pytest.mark.parametrize("order", ["deform then move", "move then deform"])
def test_deform_and_move_commute_with_the_fresh_build(frt, deformed, order):
    base, new = deformed
    moves = cornell_moves(frt)
    s = frt.scenes.create_cornell_box()
    steps = [lambda: move(s, moves)] + [lambda m=m: s.set_mesh_vertices(m, new[m].positions, new[m].attributes) for m in (CRYSTAL_MESH, PLANE, SPHERE)]
    for step in (steps[1:] + steps[:1] if order == "deform then move" else steps):
        step()
    meshes = list(base)
    for m in new:
        meshes[m] = new[m]
    assert_equals_fresh(s, cornell_with(frt, meshes, moves), order)
    check_boxes(s)


def test_wide_tree_is_not_stale(frt, deformed):
    _, new = deformed
    s = frt.scenes.create_cornell_box()
    s.get("wide8_nodes")                                                # made before the deformation
    old8, stats = s.get("tri_slots8"), _counts(s)
    s.set_mesh_vertices(SPHERE, new[SPHERE].positions, new[SPHERE].attributes)
    slots8 = s.get("tri_slots8")
    assert by_id(slots8).tobytes() == by_id(s.get("tri_slots")).tobytes()
    assert by_id(slots8).tobytes() != by_id(old8).tobytes()
    now = s.tree_stats()
    assert _counts(s) == stats
    boxes = np.zeros(now["wide8_nodes"] * 48, np.float32)
    assert frt.lib().frt_scene_get(s._h, 14, boxes.ctypes.data) == 0
    tris = s.get("tris")
    v0 = tris[:, 0:3]; v = np.concatenate([v0, v0 + tris[:, 3:6], v0 + tris[:, 6:9]])
    b = boxes.reshape(-1, 8, 6)
    valid = b[:, :, 3] >= b[:, :, 0]
    assert (b[valid][:, 0:3].min(axis=0) <= v.min(axis=0)).all() and (b[valid][:, 3:6].max(axis=0) >= v.max(axis=0)).all()


def test_errors(frt, deformed):
    base, new = deformed
    s = frt.scenes.create_cornell_box()
    before = {w: s.get(w).tobytes() for w in EVERYTHING}
    g = new[SPHERE]
    bad_pos = g.positions.copy(); bad_pos[17, 1] = np.nan
    inf_pos = g.positions.copy(); inf_pos[3, 3] = np.inf
    bad_att = g.attributes.copy(); bad_att[40, 5] = np.inf
    for args in ((4, g.positions, g.attributes),                                   # a mesh id out of range
                 (1000, g.positions, None),
                 (SPHERE, g.positions[:-1], g.attributes[:-1]),                    # a wrong vertex count
                 (PLANE, g.positions, g.attributes),
                 (SPHERE, bad_pos, g.attributes), (SPHERE, inf_pos, None),         # non-finite floats
                 (SPHERE, g.positions, bad_att)):
        with pytest.raises(frt.FrtError, match="error -1"):
            s.set_mesh_vertices(*args)
    with pytest.raises(frt.FrtError):
        s.set_mesh_vertices(SPHERE, g.positions, g.attributes[:-1])               # fewer attribute records than positions
    n = len(g.positions)
    assert frt.lib().frt_scene_set_mesh_vertices(s._h, SPHERE, None, g.attributes.ctypes.data, n) == -1      # null positions
    for w in EVERYTHING:
        assert s.get(w).tobytes() == before[w], w                                # nothing applied
    b = frt.SceneBuilder()
    b.add_mesh(base[PLANE])
    b.add_instance(0, 0xFFFFFFFF, np.eye(4, dtype=np.float32))
    with pytest.raises(frt.FrtError, match="error -4"):
        b.set_mesh_vertices(0, new[PLANE].positions)                              # not built
    assert b"not built" in frt.lib().frt_last_error()
