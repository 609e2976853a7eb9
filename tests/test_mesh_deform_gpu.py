"""Deforming meshes on the device (include/frt.h: frt_renderer_set_mesh_vertices; DESIGN.md section 11, "Deforming meshes"): the replica after the
call equals the host scene after frt_scene_set_mesh_vertices bit for bit (triangle slots, both trees, shading records), and renderers after a
deformation render exactly what a renderer over a scene built from scratch with the deformed meshes renders, and what the brute-force oracle
renders from those meshes."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes, cornell_moves, oracle_scene, by_id
from test_instance_update_gpu import gpu, _render_all      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform, cornell_with, mesh_work, PLANE, SPHERE, CRYSTAL_MESH

pytestmark = pytest.mark.gpu
REPLICA = ("tri_slots", "pair_nodes", "quad_nodes", "instances_dev", "lights", "shade_tris")
BLOCK = 256      # threads per block of mesh_deform_kernel


@pytest.fixture(scope="module")
def deformed(gpu):
    """The Cornell Box meshes and their deformed forms (mesh id -> Geometry), made once."""
    base = cornell_meshes(gpu)
    return base, {m: deform(gpu, base[m], 0.3 * m) for m in (PLANE, SPHERE, CRYSTAL_MESH)}


def _deform_all(x, new, order=(SPHERE, PLANE, CRYSTAL_MESH)):
    for m in order:
        x.set_mesh_vertices(m, new[m].positions, new[m].attributes)


def _all_new(base, new):
    meshes = list(base)
    for m in new:
        meshes[m] = new[m]
    return meshes


def _three_spheres(frt):
    """A floor, a quad light and three instances (one mirrored) of a 320-triangle sphere: one call rewrites 960 triangles, 3.75 blocks."""
    from frt.scenes import _T, _S, _RX, _mul
    g = frt.geometry
    meshes = [g.create_plane(), g.create_sphere(2)]
    b = frt.SceneBuilder()
    for m in meshes:
        b.add_mesh(m)
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(0, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.register_quad_light(0, _mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.5)), (1.0, 1.0, 1.0), 10.0)
    b.add_instance(1, grey, _mul(_T(-0.6, -0.5, 0.0), _S(0.5)))
    b.add_instance(1, grey, _mul(_T(0.6, -0.5, 0.2), np.diag(np.array([-0.4, 0.6, 0.4, 1.0], np.float32))))
    b.add_instance(1, grey, _mul(_T(0.0, 0.2, -0.5), _S(0.3)))
    return b.build(), meshes


@pytest.mark.parametrize("which", ["cornell", "restir", "three spheres"])
def test_device_replica_matches_the_host_reference(gpu, which):
    frt = gpu
    g = frt.geometry
    if which == "cornell":
        fs, meshes = frt.scenes.create_cornell_box(), cornell_meshes(frt)
    elif which == "restir":
        fs, meshes = frt.scenes.create_restir_scene(), [g.create_plane(), g.create_sphere(2), g.create_cube()]
    else:
        fs, meshes = _three_spheres(frt)
    work = [mesh_work(fs, m) for m in range(len(meshes))]
    print(f"{which}: triangles rewritten per mesh {work}")
    assert sum(work) % BLOCK and any(w % BLOCK for w in work)          # launches with a partial last block
    if which == "three spheres":
        assert any(w > BLOCK and w % BLOCK for w in work)              # ... behind full ones
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    for w in REPLICA:
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), f"{which} {w} at create"
    before = {w: r.read_scene(w).tobytes() for w in ("tri_slots", "shade_tris")}
    r.render(frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights))
    # every mesh twice in a row with no sync in between (the second call reuses the staging of the first), then positions only
    calls = []
    for m, geo in enumerate(meshes):
        calls += [(m, deform(frt, geo, 1.0 + m)), (m, deform(frt, geo, 0.3 * m))]
    for m, d in calls:
        r.set_mesh_vertices(m, d.positions, d.attributes)
    for m, d in calls:
        fs.set_mesh_vertices(m, d.positions, d.attributes)
    for w in REPLICA:
        got, want = r.read_scene(w), fs.get(w)
        assert got.tobytes() == want.tobytes(), f"{which} {w}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
    assert r.read_scene("tri_slots").tobytes() != before["tri_slots"] and r.read_scene("shade_tris").tobytes() != before["shade_tris"]
    rec = r.read_scene("shade_tris").tobytes()
    p = deform(frt, meshes[1], 2.0).positions
    r.set_mesh_vertices(1, p); fs.set_mesh_vertices(1, p)
    assert r.read_scene("shade_tris").tobytes() == rec
    for w in REPLICA:
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), f"{which} {w} after a positions-only call"


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_deformed_renderer_matches_a_fresh_build_and_the_oracle(gpu, orc, deformed, flags):
    frt = gpu
    base, new = deformed
    W, H, depth, frames = 128, 128, 8, 3
    meshes = _all_new(base, new)
    fresh = cornell_with(frt, meshes)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=depth, flags=flags)
    _render_all(frt, r, W, H, fresh.num_lights, 2)
    _deform_all(r, new)
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=flags)
    ro = oracle_scene(orc, fresh, meshes).renderer(W, H, depth, False, 16)      # brute force over the deformed meshes: nothing of either tree
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam); ro.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "deformed vs fresh build")
        compare_all(r.read_buffer, ro.read, f, "deformed vs brute-force oracle")
    st, sf, so = r.stats(), rf.stats(), ro.stats()["total"]
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"]) == (so["closest"], so["any"])


@pytest.mark.parametrize("flags", [8, 8 | 16], ids=["pipeline", "pipeline + third set"])
def test_mid_sequence_deformation_with_the_pipeline(gpu, deformed, flags):
    """Render 3 frames, deform, render 3 more: the two-stream schedule (whose next frame's G-buffer + T-trace ran ahead under the old geometry)
    equals the one-stream schedule on every buffer of every frame. With two G-buffer sets the frame running ahead writes the set of the
    previous logical slot, which a read through the ABI then shows: after a deformation it holds the new geometry's pixels, so there only the
    frame's own slot of the G-buffer targets is compared (as test_mid_sequence_move_with_the_pipeline does)."""
    frt = gpu
    _, new = deformed
    W, H = 96, 64
    fs = frt.scenes.create_cornell_box()
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H, flags=flags)
    third = bool(flags & 16)
    for f in range(6):
        if f == 3:
            _deform_all(a, new); _deform_all(b, new)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        assert a.frame_count == b.frame_count == f + 1
        for buf in range(8):
            for idx in ((0, 1) if buf in (0, 1, 2, 4, 7) else (0,)):
                if buf in (0, 1, 2) and idx != f % 2 and not third:
                    continue
                g, w = b.read_buffer(buf, idx), a.read_buffer(buf, idx)
                assert g.tobytes() == w.tobytes(), f"frame {f} buffer {buf}[{idx}]"
    sa, sb = a.stats(), b.stats()
    assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    assert sb["discarded_speculations"] >= 1          # the frame speculated under the old geometry was dropped


def test_deform_after_a_rebuild_then_move(gpu, deformed):
    """rebuild_tree("sah"), deform, move: the deformation uses the rebuilt tree's slot table and level ranges, and the move transforms the new vertices."""
    frt = gpu
    base, new = deformed
    W, H, depth = 96, 96, 8
    moves = cornell_moves(frt)
    ids = sorted(moves)
    mats = np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])
    fresh = cornell_with(frt, _all_new(base, new), moves)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    _render_all(frt, r, W, H, fresh.num_lights, 2)
    r.rebuild_tree("sah")
    _deform_all(r, new)
    r.set_instance_transforms(ids, mats)
    assert r.tree_stats()["origin"] == 2
    assert by_id(r.read_scene("tri_slots")).tobytes() == by_id(fresh.get("tri_slots")).tobytes()
    for w in ("shade_tris", "instances_dev", "lights"):
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), w
    with pytest.raises(frt.FrtError, match="error -4"):
        r.read_scene("pair_nodes")
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    for f in range(3):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "rebuild, deform, move vs fresh build")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])


def test_multi_renderer_strips_match_one_renderer(gpu, deformed):
    frt = gpu
    _, new = deformed
    W, H = 128, 96
    fs = frt.scenes.create_cornell_box()
    multi = frt.MultiRenderer(fs, W, H, [0, 0])
    one = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(4):
        if f == 2:
            _deform_all(multi, new); _deform_all(one, new)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        multi.render(cam); one.render(cam)
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    assert multi.read_display().tobytes() == one.read_display().tobytes()
    with pytest.raises(frt.FrtError, match="error -1"):
        multi.set_mesh_vertices(99, new[PLANE].positions, new[PLANE].attributes)


def test_renderer_argument_and_state_errors(gpu, deformed):
    frt = gpu
    _, new = deformed
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, 32, 32)
    g = new[SPHERE]
    bad_pos = g.positions.copy(); bad_pos[5, 2] = np.nan
    bad_att = g.attributes.copy(); bad_att[7, 0] = np.inf
    for args in ((4, g.positions, g.attributes), (SPHERE, g.positions[:-1], g.attributes[:-1]), (PLANE, g.positions, None),
                 (SPHERE, bad_pos, g.attributes), (SPHERE, g.positions, bad_att)):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.set_mesh_vertices(*args)
    assert frt.lib().frt_renderer_set_mesh_vertices(r._h, SPHERE, None, g.attributes.ctypes.data, len(g.positions)) == -1      # null positions
    cam = frt.CameraController().build_uniform(1.0, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    with pytest.raises(frt.FrtError, match="error -4"):
        r.set_mesh_vertices(SPHERE, g.positions, g.attributes)          # a frame is open
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    for w in REPLICA:
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w    # nothing applied
    r.set_mesh_vertices(SPHERE, g.positions, g.attributes)
    fs.set_mesh_vertices(SPHERE, g.positions, g.attributes)
    for w in REPLICA:
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w
