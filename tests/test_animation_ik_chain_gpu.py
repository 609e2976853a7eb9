"""Chain IK on the device (include/frt.h: FRT_GOAL_CHAIN; DESIGN.md section 11, "Chain IK"): the layered kernels' palette, weights and matrices
under chain goals are frt_rig_evaluate_layers_ik's and frt_rig_evaluate_nodes_layers_ik's, bit for bit, on the shapes at which the lane form could
go wrong (chains of 2 and 3 nodes; 32 and 31 nodes, a tip that carries 38 nodes; side branches and a member past the 256-lane stride; all of LDS
with a chain ending on the last node), at 1 and 16 sweeps, one chain, 16 overlapping ones, chains interleaved with two-bone and aim goals, with
and without masks, 1 and 8 layers, for the palette and, on the same four shapes, for the instance matrices; records the kernel must skip; a cast over bindings with a chain, with two-bone goals only and without goals;
the earlier calls ignore chain goals; what is refused enqueues nothing; a MultiRenderer's strips follow the host form. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_skin_gpu import check_replica, W, H
from test_animation_nodes_gpu import EVERY as SCENE
from test_animation_gpu import SPARE, CHARACTER, bind_synthetic
from test_animation_blend_gpu import near_identity
from test_animation_layers_gpu import _scene
from test_animation_ik_gpu import bits, targets_for, _character, _limb, _ik_world
from test_mesh_deform import PLANE
from _skin_model import F, scene_with_a_spare_mesh
from _blend_model import make_blend_rig, random_blends
from _layers_model import to_layers, random_masks, random_stacks
from _ik_model import TB, AIM
from _ik_chain_model import CH, to_goals, chain_nodes

pytestmark = pytest.mark.gpu
SHAPES = {"chains of 2 and 3 nodes": "chain3", "32 and 31 nodes, a tip that carries 38": "chain70", "side branches, past the workgroup's stride": "tree257",
          "the LDS limit": "tree1024"}
SWEEPS = (1, 16)


def path_to(par, tip, most=32):
    """The parent path that ends at `tip`, at most `most` nodes of it, top first."""
    path = [int(tip)]
    while par[path[-1]] >= 0 and len(path) < most:
        path.append(int(par[path[-1]]))
    return path[::-1]


def goal_sets(desc, s):
    """Goal lists under `s` sweeps: one chain (the path to the last node, which on the trees holds side branches and the node past the stride, and
    the shape's own edge cases); 16 chains down one path, overlapping; chains interleaved with two-bone and aim goals."""
    par = np.asarray(desc["parents"])
    n = len(par)
    dep = np.zeros(n, int)
    for k, p in enumerate(par):
        dep[k] = 0 if p < 0 else dep[p] + 1
    last, deep = path_to(par, n - 1), path_to(par, int(np.argmax(dep)))
    sets = [[CH(last[0], last[-1], s)], [CH(deep[0], deep[-1], s)]]
    if n == 3:
        sets += [[CH(0, 1, s)], [CH(1, 2, s)]]                                   # two nodes: one bone, the tip below it or a leaf
    if n == 70:
        sets += [[CH(1, 32, s)], [CH(2, 32, s)], [CH(20, 31, s)]]                # 32 nodes; 31; node 31 carries the 38 nodes below it
    p = deep
    sets.append([CH(p[i * (len(p) - 2) // 15], p[min(i * (len(p) - 2) // 15 + 1 + i % 5, len(p) - 1)], s) for i in range(16)])      # 16 chains down one path
    if len(p) >= 5:
        a, b, c, d, e = p[0], p[len(p) // 4], p[len(p) // 2], p[3 * len(p) // 4], p[-1]
        sets.append([TB(a, b, c), CH(b, d, s), AIM(d, (0.0, 1.0, 0.0)), CH(a, e, s), TB(c, d, e), CH(c, e, s), AIM(a, (1.0, 0.0, 0.0))])      # each reads what the earlier left
    else:
        sets.append([AIM(0, (0.0, 1.0, 0.0)), CH(0, 2, s), TB(0, 1, 2), CH(1, 2, s)])
    return sets


@pytest.mark.parametrize("which", list(SHAPES))
def test_palette_and_weights_have_the_host_bits(gpu, which):
    frt = gpu
    shape = SHAPES[which]
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    desc = make_blend_rig(shape, nclips=3, joints="all", num_targets=3, keys=(1, 2, 33))
    rig = frt.Rig(**desc)
    bind_synthetic(frt, r, meshes, [SPARE], rig)
    b = r.bind_rig(rig, [SPARE])
    rng = np.random.default_rng(len(shape) + 1)
    moved = calls = 0
    for masks in (None, random_masks(desc, 4, seed=3)):
        r.set_rig_masks(b, masks)
        for nl in (1, 8):
            layers = to_layers(frt, random_stacks(desc, nl, 1, "mixed", nmasks=0 if masks is None else 4, seed=nl)[0])
            plain = rig.evaluate_layers(layers, masks)
            for s in SWEEPS:
                for goals in goal_sets(desc, s):
                    rows = targets_for(goals, rng)
                    r.set_rig_goals(b, to_goals(frt, goals))
                    r.set_rig_goal_targets(b, rows)
                    r.animate_layers(b, layers)
                    got, want = r.read_rig_pose(b), rig.evaluate_layers(layers, masks, to_goals(frt, goals), rows)
                    assert bits(got[0]) == bits(want[0]), f"{which}, {nl} layers, masks {masks is not None}: palette under {goals}"
                    assert bits(got[1]) == bits(want[1]) == bits(plain[1])
                    moved += bits(want[0]) != bits(plain[0])
                    calls += 1
    assert moved == calls >= 32      # the goals did act, every time
    assert r.deform_rejects() == 0
    r.unbind_rig(b)


def test_matrices_have_the_host_bits(gpu):
    frt = gpu
    n = 257
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=2)
    rng = np.random.default_rng(n)
    mats = np.tile(np.eye(4, dtype=F).reshape(16), (n - 9, 1))
    mats[:, [0, 5, 10]] = F(0.02)
    mats[:, 12:15] = rng.uniform(-0.8, 0.8, (n - 9, 3)).astype(F)
    assert r.add_instances([PLANE] * (n - 9), [0] * (n - 9), mats) == 9
    ids = rng.permutation(n)
    for shape in SHAPES.values():      # chain3, chain70, tree257, tree1024
        desc = make_blend_rig(shape, nclips=3, joints="none", num_targets=0, keys=(1, 2, 33))
        rig = frt.Rig(**desc, nodes_only=True)
        nodes = rng.integers(0, rig.num_nodes, n)
        for masks in (None, random_masks(desc, 4, seed=n)):
            layers = to_layers(frt, random_stacks(desc, 3, 1, "mixed", nmasks=0 if masks is None else 4, seed=1)[0])
            for kw in ({}, {"root": near_identity(rng, 1)[0], "offsets": near_identity(rng, n)}):
                bnd = r.bind_rig_instances(rig, ids, nodes, **kw)
                r.set_rig_masks(bnd, masks)
                plain = rig.evaluate_nodes_layers(layers, nodes, masks=masks, **kw)
                for s in SWEEPS:
                    for goals in goal_sets(desc, s):
                        rows = targets_for(goals, rng)
                        r.set_rig_goals(bnd, to_goals(frt, goals))
                        r.set_rig_goal_targets(bnd, rows)
                        r.animate_instances_layers(bnd, layers)
                        want = rig.evaluate_nodes_layers(layers, nodes, masks=masks, goals=to_goals(frt, goals), targets=rows, **kw)
                        assert bits(r.read_rig_instances(bnd)) == bits(want) != bits(plain), f"{shape}, masks {masks is not None}, {sorted(kw)}: {goals}"
                r.unbind_rig(bnd)
    assert r.transform_rejects() == 0


def _chains(desc):
    """Two chains on the 12-node character's deepest limb: the whole limb, and its lower bone behind it."""
    limb = _limb(desc)[0]
    return [CH(limb.root, limb.tip, 8), CH(limb.mid, limb.tip, 16)]


def test_skipped_records(gpu):
    """Device rows with a NaN, a weight of 0 and a weight of 1.5 are skipped on the device as the host form skips a weight of 0; a chain behind a
    skipped one still runs (both barriers of a round are unconditional)."""
    frt = gpu
    import torch
    desc, rig, fs, meshes = _character(frt)
    r = frt.Renderer(fs, W, H)
    bind_synthetic(frt, r, meshes, CHARACTER, rig)
    b = r.bind_rig(rig, CHARACTER)
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    limb = _limb(desc)[0]
    goals = [CH(limb.root, limb.tip, 8), CH(limb.root, limb.mid, 4), CH(limb.mid, limb.tip, 16), CH(limb.root, limb.tip, 1)]
    fg = to_goals(frt, goals)
    plain = rig.evaluate_layers(layers)
    r.set_rig_goals(b, fg)
    r.animate_layers(b, layers)      # new goals are inert until targets arrive
    got = r.read_rig_pose(b)
    assert bits(got[0]) == bits(plain[0]) and bits(got[1]) == bits(plain[1])
    rows = targets_for(goals, np.random.default_rng(3), 0.3)
    dev = f"cuda:{r.device}"
    for bad in ({0: (0, np.nan)}, {0: (3, 0.0)}, {0: (3, 1.5)}, {0: (6, np.inf), 2: (3, -0.25)}, {0: (3, 0.0), 1: (3, 0.0), 2: (3, 0.0), 3: (3, 0.0)}):
        given, seen = rows.copy(), rows.copy()
        for k, (col, x) in bad.items():
            given[k, col] = x
            seen[k, 3] = 0.0      # what the host form is given for it: weight 0, skipped
        r.set_rig_goal_targets(b, torch.from_numpy(given).to(dev))
        r.animate_layers(b, layers)
        want = rig.evaluate_layers(layers, None, fg, seen)
        assert bits(r.read_rig_pose(b)[0]) == bits(want[0]), bad
        assert (bits(want[0]) == bits(plain[0])) == (len(bad) == 4), bad      # the chains behind a skipped one did run
    assert r.deform_rejects() == 0


def test_a_cast_over_chain_two_bone_and_no_goals_is_the_single_calls_and_the_host_scene(gpu):
    frt = gpu
    fs, descs, rigs, masks, ((r, b), (other, _)), goals, rows = _ik_world(frt)
    goals = {"spheres": _chains(descs["spheres"]), "props": [TB(*_limb(descs["props"])[0])]}      # a chain binding, a two-bone binding; the spare mesh has none
    rng = np.random.default_rng(12)
    rows = {k: targets_for(g, rng, 0.2) for k, g in goals.items()}
    for x in (r, other):
        for k in goals:
            x.set_rig_goals(b[k], to_goals(frt, goals[k]))
            x.set_rig_goal_targets(b[k], rows[k])
    meshes = scene_with_a_spare_mesh(frt)[1]
    bind_synthetic(frt, fs, meshes, [SPARE], rigs["spare"], seed=7)
    bind_synthetic(frt, fs, meshes, CHARACTER, rigs["spheres"])
    layers = {"spheres": to_layers(frt, random_stacks(descs["spheres"], 8, 1, "mixed", nmasks=2, seed=1)[0]),
              "props": to_layers(frt, random_stacks(descs["props"], 2, 1, "blend", nmasks=1, seed=1)[0]),
              "spare": to_layers(frt, random_stacks(descs["spare"], 3, 1, "mixed", nmasks=3, seed=1)[0])}
    r.animate_cast_layers([(b[k], layers[k]) for k in ("spheres", "props", "spare")])
    other.animate_instances_layers(b["props"], layers["props"])
    other.animate_layers(b["spare"], layers["spare"])
    other.animate_layers(b["spheres"], layers["spheres"])
    got, want = _scene(r), _scene(other)
    for x in SCENE:
        assert got[x] == want[x], x
    pose = r.read_rig_pose(b["spheres"])
    host = rigs["spheres"].evaluate_layers(layers["spheres"], masks["spheres"], to_goals(frt, goals["spheres"]), rows["spheres"])
    assert bits(pose[0]) == bits(host[0]) != bits(rigs["spheres"].evaluate_layers(layers["spheres"], masks["spheres"])[0])
    pose, host = r.read_rig_pose(b["spare"]), rigs["spare"].evaluate_layers(layers["spare"], masks["spare"])
    assert bits(pose[0]) == bits(host[0]) and bits(pose[1]) == bits(host[1])
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_layers(layers["props"], [3, 7], masks=masks["props"], goals=to_goals(frt, goals["props"]),
                                                                                              targets=rows["props"]))
    fs.animate_cast_layers([(rigs["props"], [1, 0], [3, 7], layers["props"], masks["props"], None, None, to_goals(frt, goals["props"]), rows["props"]),
                            {"rig": rigs["spare"], "mesh_ids": [SPARE], "layers": layers["spare"], "masks": masks["spare"]},
                            {"rig": rigs["spheres"], "mesh_ids": CHARACTER, "layers": layers["spheres"], "masks": masks["spheres"], "goals": to_goals(frt, goals["spheres"]),
                             "targets": rows["spheres"]}])
    check_replica(frt, r, fs, "a layered cast with a chain binding, a two-bone binding and one without goals")
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    rf = frt.Renderer(fs, W, H, max_depth=2)
    r.render(cam); rf.render(cam)
    compare_all(r.read_buffer, rf.read_buffer, 0, "a replica after a cast with chain goals vs a renderer created from the host scene")


def test_earlier_calls_ignore_chain_goals(gpu):
    frt = gpu
    desc, rig, fs, meshes = _character(frt)
    r = frt.Renderer(fs, W, H)
    bind_synthetic(frt, r, meshes, CHARACTER, rig)
    b = r.bind_rig(rig, CHARACTER)
    goals = _chains(desc)
    rows = targets_for(goals, np.random.default_rng(4), 0.3)
    rows[:, 3] = 1.0
    r.set_rig_goals(b, to_goals(frt, goals))
    r.set_rig_goal_targets(b, rows)
    r.animate(b, "c1", 0.5)
    got, want = r.read_rig_pose(b), rig.evaluate("c1", 0.5)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    blend = random_blends(desc, 3, 1, seed=2)[0]
    r.animate_blend(b, blend)
    assert bits(r.read_rig_pose(b)[0]) == bits(rig.evaluate_blend(blend)[0])
    layers = [("c1", 0.5, 1.0)]
    r.animate_layers(b, layers)      # and the layered call of the same clip applies them
    assert bits(r.read_rig_pose(b)[0]) == bits(rig.evaluate_layers(layers, None, to_goals(frt, goals), rows)[0]) != bits(want[0])
    assert r.deform_rejects() == 0


def test_refusals_enqueue_nothing(gpu):
    frt = gpu
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    desc = make_blend_rig("chain70", nclips=3, joints="all", num_targets=3, keys=(1, 2, 33))
    rig = frt.Rig(**desc)
    bind_synthetic(frt, r, meshes, [SPARE], rig)
    b = r.bind_rig(rig, [SPARE])
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    r.animate_layers(b, layers)
    start, counters = _scene(r), (r.transform_rejects(), r.deform_rejects())
    G = frt.RigGoal
    import ctypes as C
    from frt._lib import check
    from test_animation_ik_chain import bad_chains

    def raw(rows_):
        arr = (G * len(rows_))(*[G(k, a, m, t, (C.c_float * 3)(*ax), res) for k, a, m, t, ax, res in rows_])
        check(frt.lib().frt_renderer_set_rig_goals(r._h, b, len(rows_), arr))

    refused = {what: (lambda bad=bad: raw([(2, 1, 16, 32, (0, 0, 0), 0), bad])) for what, bad in bad_chains(70).items()}
    refused.update({"Chain: a 33-node path": lambda: r.set_rig_goals(b, [frt.Chain(0, 32)]), "Chain: no sweeps": lambda: r.set_rig_goals(b, [frt.Chain(0, 5, 0)]),
                    "Chain: 17 sweeps": lambda: r.set_rig_goals(b, [frt.Chain(0, 5, 17)])})
    for what, call in refused.items():
        with pytest.raises(frt.FrtError):
            call()
            pytest.fail(f"not refused: {what}")
        assert (r.transform_rejects(), r.deform_rejects()) == counters, what
    assert _scene(r) == start
    r.animate_layers(b, layers)      # the binding still has no goals: the plain pose
    got, plain = r.read_rig_pose(b), rig.evaluate_layers(layers)
    assert bits(got[0]) == bits(plain[0]) and bits(got[1]) == bits(plain[1]) and _scene(r) == start
    raw([(2, 1, 16, 32, (7, 7, 7), 0)])      # and the good row alone is taken (its axis is unused)
    assert (r.transform_rejects(), r.deform_rejects()) == counters


def test_multi_renderer(gpu):
    """Two strips on one device: the frame equals that of a single renderer under the same chain goals on the device."""
    frt = gpu
    desc, rig, fs, meshes = _character(frt)
    goals = to_goals(frt, _chains(desc))
    rows = targets_for(_chains(desc), np.random.default_rng(2), 0.3)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b = one.bind_rig(rig, CHARACTER)
    one.set_rig_goals(b, goals)
    one.set_rig_goal_targets(b, rows)
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    for step in range(2):
        if step == 0:
            multi.animate_layers(rig, CHARACTER, layers, goals=goals, targets=rows)
            one.animate_layers(b, layers)
        else:
            multi.animate_cast_layers([{"rig": rig, "mesh_ids": CHARACTER, "layers": layers, "goals": goals, "targets": rows}])
            one.animate_cast_layers([(b, layers)])
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), step
