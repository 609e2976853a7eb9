"""The refined mode of the device tree rebuild (include/frt.h: frt_renderer_rebuild_tree_ex with FRT_REBUILD_SAH; DESIGN.md section 11, "Refined
rebuild"): the same leaves in the same Morton order as the plain mode, a binary tree above them by parallel locally-ordered clustering, folded into
quad nodes largest-area-first. Judged as test_tree_rebuild_gpu.py judges the plain mode (a valid tree by tests/_tree_check.py, identical bytes from
identical device states, pixels and ray counts bit-equal to a refit-only renderer, a fresh host build and the oracle) and, in addition, by
tests/_tree_cost.py: over identical leaves its node term must be strictly below the Morton tree's, which the plain mode builds in the same test."""
import os
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell, cornell_meshes, move, oracle_scene, cornell_moves, by_id
from test_instance_update_gpu import gpu, _moves_for, _render_all      # noqa: F401  (gpu: the module's device fixture)
from test_tree_rebuild_gpu import big_moves, _args, _scene, _records, _compare_stats, _restir_fresh
from _tree_check import check_tree
from _tree_cost import tree_cost

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(r):
    return r.read_scene("quad_nodes"), r.read_scene("tri_slots")


@pytest.mark.parametrize("which", ["cornell", "restir", "blob82k", "coincident", "lone leaf", "one triangle"])
def test_refined_tree_is_valid_and_deterministic(gpu, orc, which):
    frt = gpu
    fs = _scene(frt, orc, which)
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    before = r.read_scene("tri_slots")
    r.render(frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights))
    r.rebuild_tree("sah")
    nodes, slots = _tree(r)
    got = check_tree(nodes, slots)
    print(f"{which}: host tree {fs.tree_stats()['quad_nodes']} nodes, refined tree {got}, {r.rebuild_stats()}")
    assert r.tree_stats() == dict(got, origin=2)
    assert r.rebuild_stats()["fell_back"] == 0
    assert got["quad_stack_need"] <= 31
    assert _records(slots) == _records(before), "the multiset of triangle slots changed"
    if which in ("lone leaf", "one triangle"):
        assert got["quad_nodes"] == 1 and got["quad_stack_need"] == 0
    # determinism: a second rebuild of the same device state gives the same bytes (into the other set of buffers), and a third (back into the first)
    for _ in range(2):
        r.rebuild_tree(quality="sah")
        n2, s2 = _tree(r)
        assert n2.tobytes() == nodes.tobytes() and s2.tobytes() == slots.tobytes()
    assert r.tree_stats() == dict(got, origin=2)
    # "sah" then "morton" gives the bytes of "morton" alone
    r.rebuild_tree("morton")
    assert r.tree_stats()["origin"] == 1
    m = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    m.render(frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights))
    m.rebuild_tree()
    assert r.tree_stats() == m.tree_stats()
    for a, b in zip(_tree(r), _tree(m)):
        assert a.tobytes() == b.tobytes()
    assert m.rebuild_stats()["refined_scratch_kib"] == 0      # a renderer that only uses the plain mode allocates nothing of the refined one


def _quality_case(frt, orc, which):
    """(scene at rest, moves, fresh host build in the moved pose)"""
    if which == "cornell":
        moves = big_moves(frt)
        return frt.scenes.create_cornell_box(), moves, cornell(frt, moves)
    if which == "restir":
        base = frt.scenes.create_restir_scene()
        moves = _moves_for(frt, "restir", base)
        return base, moves, _restir_fresh(frt, moves)[0]
    fs = _scene(frt, orc, "blob82k")
    return fs, {}, fs


@pytest.mark.parametrize("which", ["cornell", "restir", "blob82k"])
def test_refined_tree_costs_less_than_the_morton_tree(gpu, orc, which):
    frt = gpu
    base, moves, fresh = _quality_case(frt, orc, which)
    r = frt.Renderer(base, 32, 24, flags=frt.FLAG_PIPELINE)
    if moves:
        r.set_instance_transforms(*_args(moves))
    r.rebuild_tree("morton")
    mn, ms = _tree(r)
    r.rebuild_tree("sah")
    sn, ss = _tree(r)
    assert r.tree_stats()["origin"] == 2
    assert ss.tobytes() == ms.tobytes()                  # the same Morton order, hence the same leaves
    cm, cs, ch = tree_cost(mn, ms), tree_cost(sn, ss), tree_cost(fresh.get("quad_nodes"), fresh.get("tri_slots"))
    print(f"{which}: morton node_term {cm['node_term']:.4f} leaf_term {cm['leaf_term']:.4f} ({cm['nodes']} nodes); "
          f"refined node_term {cs['node_term']:.4f} leaf_term {cs['leaf_term']:.4f} ({cs['nodes']} nodes); "
          f"fresh host build node_term {ch['node_term']:.4f} leaf_term {ch['leaf_term']:.4f} ({ch['nodes']} nodes); {r.rebuild_stats()}")
    assert cs["root_area"] == cm["root_area"] and cs["leaves"] == cm["leaves"]
    assert cs["leaf_term"] == cm["leaf_term"]
    assert cs["node_term"] < cm["node_term"]


def _pixels_check(frt, orc, base, fresh, meshes, moves, W, H, depth, flags, frames, brute):
    """r: move + refined rebuild; a: the same move, refit only; rf: a fresh host build in the moved pose; ro: the oracle over that scene."""
    ids, mats = _args(moves)
    nl = fresh.num_lights
    r, a = frt.Renderer(base, W, H, max_depth=depth, flags=flags), frt.Renderer(base, W, H, max_depth=depth, flags=flags)
    _render_all(frt, r, W, H, nl, 2); _render_all(frt, a, W, H, nl, 2)
    r.set_instance_transforms(ids, mats); a.set_instance_transforms(ids, mats)
    fc = r.frame_count
    r.rebuild_tree("sah")
    assert r.frame_count == fc and r.tree_stats()["origin"] == 2 and a.tree_stats()["origin"] == 0
    check_tree(*_tree(r))
    for f in range(2, 4):                                 # accumulation and reservoirs kept: the sequence goes on as the refit-only renderer's does
        cam = frt.CameraController().build_uniform(W / H, f, nl)
        r.render(cam); a.render(cam)
        compare_all(r.read_buffer, a.read_buffer, f, "refined rebuild vs refit only, history kept")
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
        compare_all(r.read_buffer, a.read_buffer, f, "refined rebuild vs refit only")
        compare_all(r.read_buffer, rf.read_buffer, f, "refined rebuild vs fresh build")
        compare_all(r.read_buffer, ro.read, f, "refined rebuild vs oracle")
    _compare_stats(r, a, rf)
    so = ro.stats()["total"]
    assert (r.stats()["rays_closest"], r.stats()["rays_any"]) == (so["closest"], so["any"])


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_refined_renderer_matches_refit_fresh_build_and_oracle(gpu, orc, flags):
    frt = gpu
    moves = big_moves(frt)
    _pixels_check(frt, orc, frt.scenes.create_cornell_box(), cornell(frt, moves), cornell_meshes(frt), moves, 128, 128, 8, flags, 3, brute=True)


def test_refined_restir_scene_matches_refit_fresh_build_and_oracle(gpu, orc):
    frt = gpu
    base = frt.scenes.create_restir_scene()
    moves = _moves_for(frt, "restir", base)
    fresh, meshes = _restir_fresh(frt, moves)
    assert move(frt.scenes.create_restir_scene(), moves).get("tris").tobytes() == fresh.get("tris").tobytes()
    _pixels_check(frt, orc, base, fresh, meshes, moves, 48, 36, 8, frt.FLAG_PIPELINE, 2, brute=False)


def test_refit_after_refined_rebuild(gpu, orc):
    """Move, rebuild, move again: the second move refits the refined tree (new slot table, new level ranges, no pair levels)."""
    frt = gpu
    W, H, depth = 96, 96, 8
    first, final = big_moves(frt), cornell_moves(frt)
    fresh = cornell(frt, final)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    _render_all(frt, r, W, H, fresh.num_lights, 2)
    r.set_instance_transforms(*_args(first))
    r.rebuild_tree("sah")
    _render_all(frt, r, W, H, fresh.num_lights, 1, first=2)
    r.set_instance_transforms(*_args(final))
    slots = r.read_scene("tri_slots")
    got = check_tree(r.read_scene("quad_nodes"), slots)
    assert r.tree_stats() == dict(got, origin=2)
    assert by_id(slots).tobytes() == by_id(fresh.get("tri_slots")).tobytes()
    for w in ("instances_dev", "lights"):
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), w
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=frt.FLAG_PIPELINE)
    for f in range(3):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "move, refined rebuild, move vs fresh build")
    _compare_stats(r, rf)


def test_mid_sequence_refined_rebuild_with_the_pipeline(gpu):
    """A rebuild between frames with no move: the frame that ran ahead on the old tree is kept, and every later buffer equals an undisturbed renderer's."""
    frt = gpu
    W, H = 96, 64
    fs = frt.scenes.create_cornell_box()
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(6):
        if f in (3, 5):
            b.rebuild_tree("sah")
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "refined rebuild mid-sequence vs undisturbed")
    sa, sb = a.stats(), b.stats()
    assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    assert sb["discarded_speculations"] == sa["discarded_speculations"]      # nothing was dropped for the rebuild
    assert b.tree_stats()["origin"] == 2


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
            multi.rebuild_tree("sah")
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        multi.render(cam); one.render(cam)
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    assert multi.read_display().tobytes() == one.read_display().tobytes()
    assert frt.lib().frt_multi_renderer_rebuild_tree_ex(multi._h, 7) == -1      # an unknown mode: FRT_ERR_INVALID_ARG


def test_state_and_mode_errors(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, 32, 32)
    cam = frt.CameraController().build_uniform(1.0, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    before = r.read_scene("quad_nodes")
    with pytest.raises(frt.FrtError, match="error -4"):
        r.rebuild_tree("sah")                            # a frame is open: FRT_ERR_STATE
    assert r.tree_stats()["origin"] == 0 and r.read_scene("quad_nodes").tobytes() == before.tobytes()
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert frt.lib().frt_renderer_rebuild_tree_ex(r._h, 7) == -1      # an unknown mode: FRT_ERR_INVALID_ARG
    assert r.tree_stats()["origin"] == 0 and r.read_scene("quad_nodes").tobytes() == before.tobytes()
    assert r.read_scene("pair_nodes").tobytes() == fs.get("pair_nodes").tobytes()
    with pytest.raises(ValueError):
        r.rebuild_tree("best")
    r.rebuild_tree("sah")
    assert r.tree_stats()["origin"] == 2
    with pytest.raises(frt.FrtError, match="error -4"):
        r.read_scene("pair_nodes")                       # selector 15 after a rebuild: FRT_ERR_STATE


def test_experiments_build_refuses_the_wide_walk(gpu):
    import subprocess, sys
    exp = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib", "libfrt_exp.so")
    code = ("import sys, numpy as np; sys.path[:0] = [%r]; import frt\n"
            "fs = frt.scenes.create_cornell_box()\n"
            "r = frt.Renderer(fs, 32, 32, flags=frt.FLAG_WALK_WIDE)\n"
            "try:\n    r.rebuild_tree('sah')\n    print('ACCEPTED')\n"
            "except frt.FrtError as e:\n    print('REFUSED', e)\n"
            "print('ORIGIN', r.tree_stats()['origin'])\n"
            "q = frt.Renderer(fs, 32, 32)\nq.rebuild_tree('sah')\nprint('QUAD OK', q.tree_stats()['origin'])\n") % os.path.join(ROOT, "fast-raytracing-wgpu_amd")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FRT_LIB=exp))
    assert p.returncode == 0, p.stderr[-3000:]
    assert "REFUSED libfrt error -1" in p.stdout and "ORIGIN 0" in p.stdout and "QUAD OK 2" in p.stdout, p.stdout


def _row_scene(frt, xs):
    """One mesh of triangles side by side at the given x (test_tree_rebuild_gpu._one_mesh_scene's shape)."""
    ntris = len(xs)
    pos = np.zeros((3 * ntris, 4), np.float32)
    for t, x in enumerate(xs):
        pos[3 * t:3 * t + 3, :3] = [[x - 0.1, 0.0, -2.0], [x + 0.1, 0.0, -2.0], [x, 0.2, -2.0]]
    pos[:, 3] = 1.0
    att = np.zeros((3 * ntris, 8), np.float32); att[:, 1] = 1.0
    b = frt.SceneBuilder()
    mesh = b.add_mesh(frt.geometry.Geometry(pos, att, np.arange(3 * ntris, dtype=np.uint32)))
    mat = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(mesh, mat, np.eye(4, dtype=np.float32))
    return b.build()


def _fallback_check(frt, fs, reason):
    m = frt.Renderer(fs, 32, 24)
    m.rebuild_tree("morton")
    want = check_tree(*_tree(m))
    assert m.tree_stats() == dict(want, origin=1)
    r = frt.Renderer(fs, 32, 24)
    r.rebuild_tree("sah")
    print(f"morton tree {want}, refined call {r.rebuild_stats()}")
    assert r.tree_stats() == dict(want, origin=1)
    assert r.rebuild_stats()["fell_back"] == reason
    for a, b in zip(_tree(r), _tree(m)):
        assert a.tobytes() == b.tobytes()
    r.rebuild_tree("sah")                                # and again, into the other set of buffers
    assert r.tree_stats() == dict(want, origin=1)
    for a, b in zip(_tree(r), _tree(m)):
        assert a.tobytes() == b.tobytes()


def test_a_chain_of_40_leaves_falls_back_to_the_morton_tree(gpu):
    """80 triangles at x = 2^t: 40 leaves merge one pair per iteration (tests/test_ploc_model.py: 39 iterations, inside the bound of 48) into a tree
    of height 40, which cannot fit 31 stack entries. The call builds the Morton tree instead and says why."""
    from _ploc_model import chain_xs
    _fallback_check(gpu, _row_scene(gpu, chain_xs(80)), 2)


def test_a_clustering_that_passes_its_iteration_bound_falls_back_to_the_morton_tree(gpu):
    """120 triangles at x = 2^t: 60 leaves would take 59 iterations; the bound for 60 leaves is 48."""
    from _ploc_model import chain_xs
    _fallback_check(gpu, _row_scene(gpu, chain_xs(120)), 1)


def test_a_refined_tree_that_does_not_fit_the_stack_falls_back_to_the_morton_tree(gpu):
    """The same chain behind 2048 evenly spaced triangles: 1057 leaves start in the kernels of the large array and end in the tail kernel (tests/test_ploc_model.py: 49 iterations, bound 88), the
    finished tree is numbered, boxed and found to need more than 31 stack entries, and the Morton tree is built over the same scratch."""
    from _ploc_model import chain_behind_a_row_xs
    _fallback_check(gpu, _row_scene(gpu, chain_behind_a_row_xs()), 2)
