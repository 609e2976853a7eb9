"""Recomputed vertex normals on the device (include/frt.h: frt_renderer_set_mesh_vertices_ex, FRT_DEFORM_RECOMPUTE_NORMALS; DESIGN.md section 11,
"Recomputed normals"): after the same calls the replica equals the host scene bit for bit — triangle slots, both trees, shading records, attributes and
the decoded normals — on the host-built tree and on a rebuilt one, through a renumbering of the meshes (the per-mesh adjacency follows it), and the
frames rendered afterwards equal those of a renderer over a scene built from scratch with the resulting positions and attributes. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes, by_id
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform, cornell_with, PLANE, CUBE, SPHERE
from test_mesh_deform_gpu import _three_spheres
from test_scene_remove_gpu import decoded_normals

pytestmark = pytest.mark.gpu
REPLICA = ("tri_slots", "pair_nodes", "quad_nodes", "shade_tris", "attributes")
F = np.float32
W, H = 32, 24


def check_replica(frt, r, fs, what, rebuilt=False):
    """Bit equality with the host scene; after a device rebuild the trees are the device's own, so the slots are compared by triangle id."""
    for w in ("shade_tris", "attributes") if rebuilt else REPLICA:
        got, want = r.read_scene(w), fs.get(w)
        assert got.tobytes() == want.tobytes(), f"{what} {w}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
    if rebuilt:
        assert by_id(r.read_scene("tri_slots")).tobytes() == by_id(fs.get("tri_slots")).tobytes(), f"{what} tri_slots"
    assert r.read_scene("normals").tobytes() == decoded_normals(frt, fs.get("attributes")).tobytes(), f"{what} normals"


def _calls(frt, meshes, ids, phase):
    """Per mesh two calls in a row: positions only, then positions with attributes (uv and tangent taken from them), both with recomputed normals."""
    out = []
    for m in ids:
        a, b = deform(frt, meshes[m], phase + m), deform(frt, meshes[m], phase + 0.3 * m)
        out += [(m, a.positions, None), (m, b.positions, b.attributes)]
    return out


@pytest.mark.parametrize("which", ["cornell", "three spheres"])
def test_replica_equals_the_host_scene(gpu, which):
    frt = gpu
    if which == "cornell":      # the sphere (642 vertices: 2.5 blocks) is mesh 2 of the pools, the plane (4: less than a wave) mesh 0, the cube (24) mesh 1
        fs, meshes, ids = frt.scenes.create_cornell_box(), cornell_meshes(frt), (SPHERE, PLANE, CUBE)
        assert [len(meshes[m].positions) for m in ids] == [642, 4, 24] and fs.get("mesh_infos")[SPHERE, 0] > 0
    else:                       # three instances, one mirrored, of mesh 1 (162 vertices)
        (fs, meshes), ids = _three_spheres(frt), (1, 0)
        assert len(meshes[1].positions) % 64 and fs.get("instances")[:, 4].any()
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    before = r.read_scene("attributes").tobytes()
    calls = _calls(frt, meshes, ids, 1.0)
    for m, p, a in calls:       # no sync in between: the second call of a mesh reuses the staging and the adjacency of the first
        r.set_mesh_vertices(m, p, a, normals="recompute")
    for m, p, a in calls:
        fs.set_mesh_vertices(m, p, a, normals="recompute")
    check_replica(frt, r, fs, which)      # (reading "normals" makes the pool of decoded normals: the calls below keep it up as well)
    assert r.read_scene("attributes").tobytes() != before
    for m, p, a in _calls(frt, meshes, ids, 2.0)[:2] + [(ids[0], deform(frt, meshes[ids[0]], 0.7).positions, None)]:
        r.set_mesh_vertices(m, p, a, normals="recompute"); fs.set_mesh_vertices(m, p, a, normals="recompute")
    check_replica(frt, r, fs, f"{which}, with the pool of normals")
    r.rebuild_tree("sah")
    for m, p, a in _calls(frt, meshes, ids, 3.0):
        r.set_mesh_vertices(m, p, a, normals="recompute"); fs.set_mesh_vertices(m, p, a, normals="recompute")
    check_replica(frt, r, fs, f"{which}, after rebuild_tree", rebuilt=True)
    p = deform(frt, meshes[ids[0]], 4.0).positions      # normals="keep" beside it: positions only leaves attributes and records alone
    rec = r.read_scene("shade_tris").tobytes()
    r.set_mesh_vertices(ids[0], p); fs.set_mesh_vertices(ids[0], p)
    assert r.read_scene("shade_tris").tobytes() == rec
    check_replica(frt, r, fs, f"{which}, positions only", rebuilt=True)


def _builder(frt, meshes, used):
    """A floor, a quad light and one instance of every mesh of `used` (mesh id -> transform); the other meshes are in the pools, unused."""
    from frt.scenes import _T, _S, _RX, _mul
    b = frt.SceneBuilder()
    for g in meshes:
        b.add_mesh(g)
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(0, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.register_quad_light(0, _mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.5)), (1.0, 1.0, 1.0), 10.0)
    for m, t in used.items():
        b.add_instance(m, grey, t)
    return b.build(), grey


def test_adjacency_follows_the_mesh_ids(gpu):
    """Mesh 2 is deformed with recomputed normals (its adjacency is cached), a mesh is added and used (3), the unused mesh 1 is removed: 2 and 3 become
    1 and 2. Deforming both again must use each mesh's own adjacency: a stale list would gather the 162-vertex sphere's corners for the 42-vertex one."""
    from frt.scenes import _T, _S, _mul
    frt = gpu
    g = frt.geometry
    meshes = [g.create_plane(), g.create_crystal(), g.create_sphere(2)]
    small = g.create_sphere(1)
    t2, t3 = _mul(_T(-0.5, -0.4, 0.0), _S(0.6)), _mul(_T(0.5, -0.4, 0.1), np.diag(np.array([-0.5, 0.5, 0.5, 1.0], F)))
    fs, grey = _builder(frt, meshes, {2: t2})
    r = frt.Renderer(fs, W, H)
    d = deform(frt, meshes[2], 0.5)
    r.set_mesh_vertices(2, d.positions, normals="recompute"); fs.set_mesh_vertices(2, d.positions, normals="recompute")
    check_replica(frt, r, fs, "before the edits")
    assert r.add_meshes(small) == 3
    r.add_instances([3], [grey], [t3], quality="sah")
    d3 = deform(frt, small, 0.9)
    r.set_mesh_vertices(3, d3.positions, normals="recompute")      # (cached as mesh 3)
    r.remove_meshes(1)
    e2, e3 = deform(frt, meshes[2], 1.5), deform(frt, small, 1.9)
    r.set_mesh_vertices(1, e2.positions, normals="recompute")
    r.set_mesh_vertices(2, e3.positions, e3.attributes, normals="recompute")
    # the host scene given the same builder edits: built from scratch without the crystal, then the same two deformations
    want, _ = _builder(frt, [meshes[0], meshes[2], small], {1: t2, 2: t3})
    want.set_mesh_vertices(1, e2.positions, normals="recompute")
    want.set_mesh_vertices(2, e3.positions, e3.attributes, normals="recompute")
    assert r.pool_counts()["meshes"] == 3
    for w in ("indices", "mesh_infos"):
        assert r.read_scene(w).tobytes() == want.get(w).tobytes(), w
    check_replica(frt, r, want, "after add_meshes and remove_meshes", rebuilt=True)


def test_frames_equal_a_scene_built_from_scratch(gpu):
    frt = gpu
    base = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
    meshes = list(base)
    for m in (SPHERE, CUBE):
        p = deform(frt, base[m], 0.4 + m).positions
        r.set_mesh_vertices(m, p, normals="recompute"); fs.set_mesh_vertices(m, p, normals="recompute")
        mi = fs.get("mesh_infos")[m]
        meshes[m] = frt.geometry.Geometry(p, fs.get("attributes")[mi[0]:mi[0] + len(p)].copy(), base[m].indices)
    fresh = cornell_with(frt, meshes)
    assert fresh.get("shade_tris").tobytes() == fs.get("shade_tris").tobytes()
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(3):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "recomputed normals vs a build from scratch")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])


def test_multi_renderer_and_refusals(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    p = deform(frt, cornell_meshes(frt)[SPHERE], 0.2).positions
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        x.set_mesh_vertices(SPHERE, p, normals="recompute")
        x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    before = {w: one.read_scene(w).tobytes() for w in REPLICA}
    q = np.ascontiguousarray(p, F)
    assert frt.lib().frt_renderer_set_mesh_vertices_ex(one._h, SPHERE, q.ctypes.data, None, len(q), 4) == -1            # an unknown flag bit
    assert frt.lib().frt_multi_renderer_set_mesh_vertices_ex(multi._h, SPHERE, q.ctypes.data, None, len(q), 2) == -1    # the device flag on strips
    bad = q.copy(); bad[3, 1] = np.inf
    with pytest.raises(frt.FrtError, match="error -1"):
        one.set_mesh_vertices(SPHERE, bad, normals="recompute")
    with pytest.raises(frt.FrtError, match="normals must be"):
        one.set_mesh_vertices(SPHERE, q, normals="smooth")
    for w in REPLICA:
        assert one.read_scene(w).tobytes() == before[w], w
