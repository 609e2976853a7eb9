"""Rebuilding a renderer's quad tree on the device (include/frt.h: frt_renderer_rebuild_tree; DESIGN.md section 11, "Rebuild"). Hits are defined
without reference to any tree and ties are broken by flattened triangle id, so a renderer after a rebuild must render, bit for
bit, what a renderer that only refit renders, what a renderer over a freshly host-built scene renders and what the oracle renders; the tree itself is
judged by tests/_tree_check.py, which knows nothing of how it was made."""
import os
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell, cornell_meshes, move, oracle_scene, TALL_BOX, SPHERE_LIGHT
from test_instance_update_gpu import gpu, _moves_for, _render_all      # noqa: F401  (gpu: the module's device fixture)
from _tree_check import check_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def big_moves(frt):
    """The tall box across the room, turned and stretched; the sphere light from one corner to the opposite one, enlarged."""
    from frt.scenes import _T, _S, _RY, _mul
    S3 = lambda x, y, z: np.diag(np.array([x, y, z, 1.0], np.float32))
    return {TALL_BOX: _mul(_T(0.45, -0.398, 0.35), _RY(2.1), S3(0.5, 1.5, 0.5)), SPHERE_LIGHT: _mul(_T(-0.55, 0.55, -0.45), _S(0.22))}


def _args(moves):
    ids = sorted(moves)
    return ids, np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])


def _one_mesh_scene(frt, ntris, spread):
    """`ntris` triangles in one mesh: coincident (every centroid, hence every Morton code, equal) or, with `spread`, side by side."""
    pos = np.zeros((3 * ntris, 4), np.float32)
    for t in range(ntris):
        x = 0.3 * t if spread else 0.0
        pos[3 * t:3 * t + 3, :3] = [[x - 0.1, 0.0, -2.0], [x + 0.1, 0.0, -2.0], [x, 0.2, -2.0]]
    pos[:, 3] = 1.0
    att = np.zeros((3 * ntris, 8), np.float32); att[:, 1] = 1.0
    b = frt.SceneBuilder()
    mesh = b.add_mesh(frt.geometry.Geometry(pos, att, np.arange(3 * ntris, dtype=np.uint32)))
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(mesh, mat, np.eye(4, dtype=np.float32))
    return b.build()


def _scene(frt, orc, which):
    import _scenes
    if which == "cornell":
        return frt.scenes.create_cornell_box()
    if which == "restir":
        return frt.scenes.create_restir_scene()
    if which == "blob82k":
        return _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)[0]
    if which == "coincident":
        return _one_mesh_scene(frt, 301, False)
    return _one_mesh_scene(frt, 2 if which == "lone leaf" else 1, True)


def _records(slots):
    rows = np.ascontiguousarray(slots).view(np.uint32).reshape(len(slots), 12)
    return rows[np.lexsort(rows.T[::-1])].tobytes()


@pytest.mark.parametrize("which", ["cornell", "restir", "blob82k", "coincident", "lone leaf", "one triangle"])
def test_rebuilt_tree_is_valid_and_deterministic(gpu, orc, which):
    frt = gpu
    fs = _scene(frt, orc, which)
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    host = r.tree_stats()
    assert host == {"quad_nodes": fs.tree_stats()["quad_nodes"], "quad_stack_need": fs.tree_stats()["quad_stack_need"], "quad_levels": host["quad_levels"], "origin": 0}
    assert check_tree(r.read_scene("quad_nodes"), r.read_scene("tri_slots"))["quad_levels"] == host["quad_levels"]
    before = r.read_scene("tri_slots")
    r.render(frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights))
    r.rebuild_tree()
    nodes, slots = r.read_scene("quad_nodes"), r.read_scene("tri_slots")
    got = check_tree(nodes, slots)
    print(f"{which}: host tree {host}, device tree {got}")
    assert r.tree_stats() == dict(got, origin=1)
    assert got["quad_stack_need"] <= 31
    assert _records(slots) == _records(before), "the multiset of triangle slots changed"
    if which in ("lone leaf", "one triangle"):
        assert got["quad_nodes"] == 1 and got["quad_stack_need"] == 0
    elif which != "coincident":
        assert slots.tobytes() != before.tobytes()      # (a Morton order, not the host's leaf order)
    # determinism: a second rebuild of the same device state gives the same bytes (into the other set of buffers)
    r.rebuild_tree()
    assert r.read_scene("quad_nodes").tobytes() == nodes.tobytes() and r.read_scene("tri_slots").tobytes() == slots.tobytes()
    r.rebuild_tree()                                     # ... and a third, back into the first set
    assert r.read_scene("quad_nodes").tobytes() == nodes.tobytes() and r.read_scene("tri_slots").tobytes() == slots.tobytes()
    assert r.tree_stats() == dict(got, origin=1)


def _compare_stats(*renderers):
    s = [x.stats() for x in renderers]
    assert len({(x["rays_closest"], x["rays_any"]) for x in s}) == 1, [(x["rays_closest"], x["rays_any"]) for x in s]


def _pixels_check(frt, orc, base, fresh, meshes, moves, W, H, depth, flags, frames, brute):
    """r: move + rebuild; a: the same move, refit only; rf: a fresh host build in the moved pose; ro: the oracle over that scene."""
    ids, mats = _args(moves)
    nl = fresh.num_lights
    r, a = frt.Renderer(base, W, H, max_depth=depth, flags=flags), frt.Renderer(base, W, H, max_depth=depth, flags=flags)
    _render_all(frt, r, W, H, nl, 2); _render_all(frt, a, W, H, nl, 2)
    r.set_instance_transforms(ids, mats); a.set_instance_transforms(ids, mats)
    fc = r.frame_count
    r.rebuild_tree()
    assert r.frame_count == fc and r.tree_stats()["origin"] == 1 and a.tree_stats()["origin"] == 0
    check_tree(r.read_scene("quad_nodes"), r.read_scene("tri_slots"))
    for f in range(2, 4):                                 # accumulation and reservoirs kept: the sequence goes on as the refit-only renderer's does
        cam = frt.CameraController().build_uniform(W / H, f, nl)
        r.render(cam); a.render(cam)
        compare_all(r.read_buffer, a.read_buffer, f, "rebuilt vs refit only, history kept")
    _compare_stats(r, a)
    r.clear(); a.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=flags)
    osc = oracle_scene(orc, fresh, meshes)
    if not brute:
        osc.set_bvh(fresh.get("bvh2_nodes"), fresh.get("bvh2_tri_index"))      # the fresh HOST tree: nothing of the device rebuild
    ro = osc.renderer(W, H, depth, not brute, 16)
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, nl)
        for x in (r, a, rf, ro):
            x.render(cam)
        compare_all(r.read_buffer, a.read_buffer, f, "rebuilt vs refit only")
        compare_all(r.read_buffer, rf.read_buffer, f, "rebuilt vs fresh build")
        compare_all(r.read_buffer, ro.read, f, "rebuilt vs oracle")
    _compare_stats(r, a, rf)
    so = ro.stats()["total"]
    assert (r.stats()["rays_closest"], r.stats()["rays_any"]) == (so["closest"], so["any"])


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_rebuilt_renderer_matches_refit_fresh_build_and_oracle(gpu, orc, flags):
    frt = gpu
    moves = big_moves(frt)
    _pixels_check(frt, orc, frt.scenes.create_cornell_box(), cornell(frt, moves), cornell_meshes(frt), moves, 128, 128, 8, flags, 3, brute=True)


def _restir_fresh(frt, moves):
    """The ReSTIR scene issued call by call with instance k at moves[k] (its lights were added with add_light: they stay where they are)."""
    ref = frt.scenes.create_restir_scene()
    g = frt.geometry
    meshes = [g.create_plane(), g.create_sphere(2), g.create_cube()]
    b = frt.SceneBuilder()
    for m in meshes:
        b.add_mesh(m)
    for row in ref.get("materials"):
        b.add_material(frt.Material.from_buffer_copy(np.ascontiguousarray(row).tobytes()))
    for k, row in enumerate(ref.get("instances")):
        b.add_instance(int(row[0]), int(row[1]), np.asarray(moves[k], np.float32).reshape(16) if k in moves else row[5:21].view(np.float32))
    for row in ref.get("lights"):
        b.add_light(frt.Light.from_buffer_copy(np.ascontiguousarray(row).tobytes()))
    return b.build(), meshes


def test_rebuilt_restir_scene_matches_refit_fresh_build_and_oracle(gpu, orc):
    frt = gpu
    base = frt.scenes.create_restir_scene()
    moves = _moves_for(frt, "restir", base)
    fresh, meshes = _restir_fresh(frt, moves)
    assert move(frt.scenes.create_restir_scene(), moves).get("tris").tobytes() == fresh.get("tris").tobytes()
    _pixels_check(frt, orc, base, fresh, meshes, moves, 48, 36, 8, frt.FLAG_PIPELINE, 2, brute=False)


def test_refit_after_rebuild(gpu, orc):
    """Move, rebuild, move again: the second move runs on the new tree (new slot table, new level ranges, no pair levels)."""
    frt = gpu
    W, H, depth = 96, 96, 8
    from test_instance_update import cornell_moves
    first, final = big_moves(frt), cornell_moves(frt)
    fresh = cornell(frt, final)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    _render_all(frt, r, W, H, fresh.num_lights, 2)
    r.set_instance_transforms(*_args(first))
    r.rebuild_tree()
    _render_all(frt, r, W, H, fresh.num_lights, 1, first=2)
    r.set_instance_transforms(*_args(final))
    slots = r.read_scene("tri_slots")
    got = check_tree(r.read_scene("quad_nodes"), slots)
    assert r.tree_stats() == dict(got, origin=1)
    from test_instance_update import by_id
    assert by_id(slots).tobytes() == by_id(fresh.get("tri_slots")).tobytes()
    for w in ("instances_dev", "lights"):
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), w
    with pytest.raises(frt.FrtError):
        r.read_scene("pair_nodes")                       # selector 15: the pair tree is not rebuilt
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    for f in range(3):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "move, rebuild, move vs fresh build")
    _compare_stats(r, rf)


@pytest.mark.parametrize("flags", [8, 8 | 16], ids=["pipeline", "pipeline + third set"])
def test_mid_sequence_rebuild_with_the_pipeline(gpu, flags):
    """A rebuild between frames with no move: the frame that ran ahead on the old tree is kept, and every later buffer equals an undisturbed renderer's."""
    frt = gpu
    W, H = 96, 64
    fs = frt.scenes.create_cornell_box()
    a, b = frt.Renderer(fs, W, H, flags=flags), frt.Renderer(fs, W, H, flags=flags)
    for f in range(6):
        if f in (3, 5):
            b.rebuild_tree()
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "rebuilt mid-sequence vs undisturbed")
    sa, sb = a.stats(), b.stats()
    assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    assert sb["discarded_speculations"] == sa["discarded_speculations"]      # nothing was dropped for the rebuild


def test_multi_renderer_strips_match_one_renderer(gpu):
    frt = gpu
    W, H = 128, 96
    fs = frt.scenes.create_cornell_box()
    ids, mats = _args(big_moves(frt))
    multi = frt.MultiRenderer(fs, W, H, [0, 0])
    one = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(5):
        if f == 2:
            multi.set_instance_transforms(ids, mats); one.set_instance_transforms(ids, mats)
            multi.rebuild_tree()
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        multi.render(cam); one.render(cam)
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    assert multi.read_display().tobytes() == one.read_display().tobytes()


def test_state_errors(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, 32, 32)
    cam = frt.CameraController().build_uniform(1.0, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    before = r.read_scene("quad_nodes")
    with pytest.raises(frt.FrtError, match="error -4"):
        r.rebuild_tree()                                 # a frame is open: FRT_ERR_STATE
    assert r.tree_stats()["origin"] == 0 and r.read_scene("quad_nodes").tobytes() == before.tobytes()
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert r.read_scene("pair_nodes").tobytes() == fs.get("pair_nodes").tobytes()
    r.rebuild_tree()
    with pytest.raises(frt.FrtError, match="error -4"):
        r.read_scene("pair_nodes")                       # selector 15 after a rebuild: FRT_ERR_STATE


def test_experiments_build_refuses_the_wide_walk(gpu):
    import subprocess, sys
    exp = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib", "libfrt_exp.so")
    code = ("import sys, numpy as np; sys.path[:0] = [%r]; import frt\n"
            "fs = frt.scenes.create_cornell_box()\n"
            "r = frt.Renderer(fs, 32, 32, flags=frt.FLAG_WALK_WIDE)\n"
            "try:\n    r.rebuild_tree()\n    print('ACCEPTED')\n"
            "except frt.FrtError as e:\n    print('REFUSED', e)\n"
            "print('ORIGIN', r.tree_stats()['origin'])\n"
            "q = frt.Renderer(fs, 32, 32)\nq.rebuild_tree()\nprint('QUAD OK', q.tree_stats()['origin'])\n") % os.path.join(ROOT, "fast-raytracing-wgpu_amd")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FRT_LIB=exp))
    assert p.returncode == 0, p.stderr[-3000:]
    assert "REFUSED libfrt error -1" in p.stdout and "ORIGIN 0" in p.stdout and "QUAD OK 1" in p.stdout, p.stdout
