"""Inverse kinematics on the device (include/frt.h: frt_renderer_set_rig_goals, _set_rig_goal_targets; DESIGN.md section 11, "Inverse kinematics"):
the layered kernels' palette, weights and matrices under a binding's goals are frt_rig_evaluate_layers_ik's and frt_rig_evaluate_nodes_layers_ik's,
bit for bit, on the rig shapes at which the goal rounds could go wrong (a limb of three nodes, a 60-node subtree, membership past the 256 lanes, all
of LDS), for 1, 2 and 16 goals of both kinds, chained and overlapping, with and without masks, 1 and 8 layers; records the kernel must skip; goals
and targets in stream order, from host and from device memory; a cast over bindings with and without goals; the earlier calls ignore goals; what is
refused enqueues nothing; a MultiRenderer's strips follow the host form. Tiny frames."""
import ctypes as C
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_skin_gpu import check_replica, W, H
from test_animation_nodes_gpu import EVERY as SCENE
from test_animation_gpu import SPARE, CHARACTER, bind_synthetic
from test_animation_blend_gpu import character_blend_rig, near_identity
from test_animation_layers_gpu import _cast_world, _scene
from test_mesh_deform import PLANE
from _skin_model import F, scene_with_a_spare_mesh
from _blend_model import make_blend_rig, random_blends
from _layers_model import to_layers, random_masks, random_stacks
from _ik_model import TB, AIM, to_goals, random_goals

pytestmark = pytest.mark.gpu
GOAL_COUNTS = (1, 2, 16)
# a limb of three nodes; a goal high in the chain moves a 60-node subtree; membership strides past the 256 lanes; all of LDS
SHAPES = {"chain3": "chain3", "a 60-node subtree": "chain70", "past the workgroup's stride": "tree257", "the LDS limit": "tree1024"}


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def targets_for(goals, rng, scale=1.0):
    """[G, 8]: targets about the origin, weights 1, 0.5 and random in turn, a pole on every second two-bone goal."""
    rows = np.zeros((len(goals), 8), F)
    for k, g in enumerate(goals):
        rows[k, :3] = scale * rng.standard_normal(3)
        rows[k, 3] = (1.0, 0.5, rng.uniform(0.1, 1.0))[k % 3]
        if isinstance(g, TB) and k % 4 >= 2:
            rows[k, 4:7], rows[k, 7] = scale * rng.standard_normal(3), 1.0
    return rows


def goal_sets(desc, rng):
    """Goal lists of 1, 2 and 16 goals of both kinds; with the 60-node subtree, a root node and a leaf tip among them."""
    par = np.asarray(desc["parents"])
    n = len(par)
    sets = [random_goals(desc, ng, rng) for ng in GOAL_COUNTS]
    leaf = n - 1      # (the last node has no children: parents come first)
    if n >= 3 and par[leaf] >= 0 and par[par[leaf]] >= 0:
        chain = [leaf]
        while par[chain[-1]] >= 0:
            chain.append(int(par[chain[-1]]))
        sets.append([TB(chain[-1], chain[len(chain) // 2], leaf), AIM(chain[-1], (0.0, 1.0, 0.0)), AIM(leaf, (1.0, 0.0, 0.0))])      # a goal on a root; a tip that is a leaf
    if n == 70:
        sets.append([TB(5, 9, 40), AIM(9), TB(9, 30, 69)])      # node 9 of the chain carries the 60 nodes below it; chained and overlapping
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
    rng = np.random.default_rng(len(shape))
    moved = 0
    for masks in (None, random_masks(desc, 4, seed=3)):
        r.set_rig_masks(b, masks)
        for nl in (1, 8):
            layers = to_layers(frt, random_stacks(desc, nl, 1, "mixed", nmasks=0 if masks is None else 4, seed=nl)[0])
            plain = rig.evaluate_layers(layers, masks)
            for goals in goal_sets(desc, rng):
                rows = targets_for(goals, rng)
                r.set_rig_goals(b, to_goals(frt, goals))
                r.set_rig_goal_targets(b, rows)
                r.animate_layers(b, layers)
                got, want = r.read_rig_pose(b), rig.evaluate_layers(layers, masks, to_goals(frt, goals), rows)
                assert bits(got[0]) == bits(want[0]), f"{which}, {nl} layers, masks {masks is not None}: palette under {goals}"
                assert bits(got[1]) == bits(want[1]) == bits(plain[1])
                moved += bits(want[0]) != bits(plain[0])
    assert moved >= 8      # the goals did act
    r.unbind_rig(b)


@pytest.mark.parametrize("n", (1, 257))
def test_matrices_have_the_host_bits(gpu, n):
    frt = gpu
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=2)
    rng = np.random.default_rng(n)
    if n > 9:
        mats = np.tile(np.eye(4, dtype=F).reshape(16), (n - 9, 1))
        mats[:, [0, 5, 10]] = F(0.02)
        mats[:, 12:15] = rng.uniform(-0.8, 0.8, (n - 9, 3)).astype(F)
        assert r.add_instances([PLANE] * (n - 9), [0] * (n - 9), mats) == 9
    ids = [8] if n == 1 else rng.permutation(n)
    for shape in ("chain70", "tree257"):
        desc = make_blend_rig(shape, nclips=3, joints="none", num_targets=0, keys=(1, 2, 33))
        rig = frt.Rig(**desc, nodes_only=True)
        nodes = rng.integers(0, rig.num_nodes, n)
        masks = random_masks(desc, 4, seed=n)
        layers = to_layers(frt, random_stacks(desc, 3, 1, "mixed", nmasks=4, seed=1)[0])
        for kw in ({}, {"root": near_identity(rng, 1)[0], "offsets": near_identity(rng, n)}):
            bnd = r.bind_rig_instances(rig, ids, nodes, **kw)
            r.set_rig_masks(bnd, masks)
            for goals in goal_sets(desc, rng):
                rows = targets_for(goals, rng)
                r.set_rig_goals(bnd, to_goals(frt, goals))
                r.set_rig_goal_targets(bnd, rows)
                r.animate_instances_layers(bnd, layers)
                want = rig.evaluate_nodes_layers(layers, nodes, masks=masks, goals=to_goals(frt, goals), targets=rows, **kw)
                assert bits(r.read_rig_instances(bnd)) == bits(want), f"{shape}, n {n}, {sorted(kw)}: {goals}"
            r.unbind_rig(bnd)


def _character(frt, extra=()):
    desc = character_blend_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    return desc, rig, fs, meshes


def _limb(desc):
    """A two-bone limb and an aim on its tip in the 12-node character: the deepest node, its parent and grandparent."""
    par = np.asarray(desc["parents"])
    dep = np.zeros(len(par), int)
    for k, p in enumerate(par):
        dep[k] = 0 if p < 0 else dep[p] + 1
    tip = int(np.argmax(dep))
    return [TB(int(par[par[tip]]), int(par[tip]), tip), AIM(tip, (0.0, 0.0, 1.0))]


def test_skipped_records(gpu):
    """Goals set but every weight 0: the bits of the plain layered call. A device tensor with a NaN row and an infinite row: those goals are
    skipped on the device and the rest applied, the bits of the host form given the same rows with the bad ones at weight 0."""
    frt = gpu
    import torch
    desc, rig, fs, meshes = _character(frt)
    r = frt.Renderer(fs, W, H)
    bind_synthetic(frt, r, meshes, CHARACTER, rig)
    b = r.bind_rig(rig, CHARACTER)
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    goals = _limb(desc) + [AIM(0, (1.0, 0.0, 0.0)), AIM(3, (0.0, 1.0, 0.0))]
    plain = rig.evaluate_layers(layers)
    r.set_rig_goals(b, to_goals(frt, goals))
    r.animate_layers(b, layers)      # new goals are inert until targets arrive
    got = r.read_rig_pose(b)
    assert bits(got[0]) == bits(plain[0]) and bits(got[1]) == bits(plain[1])
    rows = targets_for(goals, np.random.default_rng(3), 0.3)
    zero = rows.copy()
    zero[:, 3] = 0.0
    r.set_rig_goal_targets(b, zero)
    r.animate_layers(b, layers)
    assert bits(r.read_rig_pose(b)[0]) == bits(plain[0])
    bad = rows.copy()
    bad[1, 0], bad[2, 5] = np.nan, np.inf      # goal 1: a NaN target word; goal 2: an infinite pole word
    seen = rows.copy()
    seen[1, 3] = seen[2, 3] = 0.0              # what the host form is given for them: weight 0, skipped
    dev = torch.from_numpy(bad).to(f"cuda:{r.device}")
    r.set_rig_goal_targets(b, dev)
    r.animate_layers(b, layers)
    want = rig.evaluate_layers(layers, None, to_goals(frt, goals), seen)
    assert bits(r.read_rig_pose(b)[0]) == bits(want[0]) != bits(plain[0])
    over = rows.copy()
    over[0, 3], over[3, 3] = 1.5, -0.25        # weights outside (0, 1]: skipped on the device
    seen = rows.copy()
    seen[0, 3] = seen[3, 3] = 0.0
    r.set_rig_goal_targets(b, torch.from_numpy(over).to(f"cuda:{r.device}"))
    r.animate_layers(b, layers)
    assert bits(r.read_rig_pose(b)[0]) == bits(rig.evaluate_layers(layers, None, to_goals(frt, goals), seen)[0])
    assert r.deform_rejects() == 0


def test_goals_and_targets_act_in_stream_order(gpu):
    frt = gpu
    import torch
    desc, rig, fs, meshes = _character(frt)
    r, twin = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    for x in (r, twin, fs):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    goals = to_goals(frt, _limb(desc))
    rng = np.random.default_rng(5)
    first, second = targets_for(_limb(desc), rng, 0.3), targets_for(_limb(desc), rng, 0.3)
    layers = [("c0", 0.4, 1.0), frt.Layer("c2", 0.6, 0.7, mode="additive", reference=("c2", 0.3))]
    b, tb = r.bind_rig(rig, CHARACTER), twin.bind_rig(rig, CHARACTER)
    r.set_rig_goals(b, goals); twin.set_rig_goals(tb, goals)
    r.set_rig_goal_targets(b, first)
    r.animate_layers(b, layers)
    r.set_rig_goal_targets(b, second)
    r.animate_layers(b, layers)      # no wait between the four calls
    twin.set_rig_goal_targets(tb, first)
    twin.animate_layers(tb, layers)
    want1, want2 = rig.evaluate_layers(layers, None, goals, first), rig.evaluate_layers(layers, None, goals, second)
    assert bits(want1[0]) != bits(want2[0])
    assert bits(r.read_rig_pose(b)[0]) == bits(want2[0]) and bits(twin.read_rig_pose(tb)[0]) == bits(want1[0])
    fs.animate_layers(rig, CHARACTER, layers, goals=goals, targets=first)
    fs.animate_layers(rig, CHARACTER, layers, goals=goals, targets=second)
    check_replica(frt, r, fs, "two layered calls with a change of targets between them")
    # the same with device tensors written on the caller's stream just before each call
    dev = f"cuda:{r.device}"
    t1 = torch.from_numpy(first).to(dev)
    r.set_rig_goal_targets(b, t1)
    r.animate_layers(b, layers)
    t2 = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    t2.copy_(torch.from_numpy(second).to(dev))
    r.set_rig_goal_targets(b, t2)
    del t2      # (the renderer holds it until its stream has passed the call)
    r.animate_layers(b, layers)
    assert bits(r.read_rig_pose(b)[0]) == bits(want2[0])
    r.set_rig_goal_targets(b, t1)
    r.animate_layers(b, layers)
    r.set_rig_goals(b, None)         # cleared between two calls: the plain bits
    r.animate_layers(b, layers)
    assert bits(r.read_rig_pose(b)[0]) == bits(rig.evaluate_layers(layers)[0])
    assert r.deform_rejects() == 0


def _ik_world(frt):
    """_cast_world with goals on the spheres' mesh binding and on the props' instance binding; the spare mesh's binding has none."""
    fs, descs, rigs, masks, pair = _cast_world(frt)
    rng = np.random.default_rng(11)
    goals = {"spheres": _limb(descs["spheres"]), "props": [AIM(3, (0.0, 1.0, 0.0)), TB(*_limb(descs["props"])[0])]}
    rows = {k: targets_for(g, rng, 0.2) for k, g in goals.items()}
    return fs, descs, rigs, masks, pair, goals, rows


def test_a_cast_with_goals_is_the_single_calls_and_the_host_scene(gpu):
    frt = gpu
    fs, descs, rigs, masks, ((r, b), (other, _)), goals, rows = _ik_world(frt)
    for x in (r, other):
        for k in goals:
            x.set_rig_goals(b[k], to_goals(frt, goals[k]))
            x.set_rig_goal_targets(b[k], rows[k])
    meshes = scene_with_a_spare_mesh(frt)[1]      # (the geometry; the host scene gets what _cast_world gave the renderers)
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
    assert bits(pose[0]) == bits(host[0]) and bits(pose[1]) == bits(host[1])      # the entry without goals runs the loop zero times
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_layers(layers["props"], [3, 7], masks=masks["props"], goals=to_goals(frt, goals["props"]),
                                                                                              targets=rows["props"]))
    fs.animate_cast_layers([(rigs["props"], [1, 0], [3, 7], layers["props"], masks["props"], None, None, to_goals(frt, goals["props"]), rows["props"]),
                            {"rig": rigs["spare"], "mesh_ids": [SPARE], "layers": layers["spare"], "masks": masks["spare"]},
                            {"rig": rigs["spheres"], "mesh_ids": CHARACTER, "layers": layers["spheres"], "masks": masks["spheres"], "goals": to_goals(frt, goals["spheres"]),
                             "targets": rows["spheres"]}])
    check_replica(frt, r, fs, "a layered cast with goals")
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    rf = frt.Renderer(fs, W, H, max_depth=2)
    r.render(cam); rf.render(cam)
    compare_all(r.read_buffer, rf.read_buffer, 0, "a replica after a cast with goals vs a renderer created from the host scene")


def test_earlier_calls_ignore_goals(gpu):
    frt = gpu
    fs, descs, rigs, masks, ((r, b), _), goals, rows = _ik_world(frt)
    for k in goals:
        r.set_rig_goals(b[k], to_goals(frt, goals[k]))
        full = rows[k].copy()
        full[:, 3] = 1.0
        r.set_rig_goal_targets(b[k], full)
    rig, desc = rigs["spheres"], descs["spheres"]
    r.animate(b["spheres"], "c1", 0.5)
    got, want = r.read_rig_pose(b["spheres"]), rig.evaluate("c1", 0.5)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    blend = random_blends(desc, 3, 1, seed=2)[0]
    r.animate_blend(b["spheres"], blend)
    assert bits(r.read_rig_pose(b["spheres"])[0]) == bits(rig.evaluate_blend(blend)[0])
    r.animate_instances(b["props"], "c2", 0.45)
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes("c2", 0.45, [3, 7]))
    moves = random_blends(descs["props"], 2, 1, seed=3)[0]
    r.animate_instances_blend(b["props"], moves)
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_blend(moves, [3, 7]))
    r.animate_cast([(b["props"], "c1", 0.5), (b["spheres"], "c0", 0.4)])
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes("c1", 0.5, [3, 7]))
    assert bits(r.read_rig_pose(b["spheres"])[0]) == bits(rig.evaluate("c0", 0.4)[0])
    r.animate_cast_blend([(b["props"], moves), (b["spheres"], blend)])
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_blend(moves, [3, 7]))
    assert bits(r.read_rig_pose(b["spheres"])[0]) == bits(rig.evaluate_blend(blend)[0])
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0)


def test_refusals_enqueue_nothing(gpu):
    frt = gpu
    import torch
    from frt._lib import check
    from test_animation_ik import bad_goals, bad_targets
    lib = frt.lib()
    fs, descs, rigs, masks, ((r, b), (twin, _)), goals, rows = _ik_world(frt)
    mesh = b["spheres"]
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mask=1, mode="override")]
    for x in (r, twin):
        x.set_rig_goals(mesh, to_goals(frt, goals["spheres"]))
        x.set_rig_goal_targets(mesh, rows["spheres"])
        x.animate_layers(mesh, layers)
    start, counters, pose = _scene(r), (r.transform_rejects(), r.deform_rejects()), r.read_rig_pose(mesh)
    G, T = frt.RigGoal, frt.RigGoalTarget
    limb = goals["spheres"][0]

    def set_goals(table, n=None, binding=mesh, null=False):
        arr = (G * max(len(table), 1))(*[G(k, a, m, t, (C.c_float * 3)(*ax), res) for k, a, m, t, ax, res in table])
        check(lib.frt_renderer_set_rig_goals(r._h, binding, len(table) if n is None else n, None if null else arr))

    def set_targets(t, n=None, binding=mesh, flags=0, ptr=None):
        t = np.ascontiguousarray(t, F)
        check(lib.frt_renderer_set_rig_goal_targets(r._h, binding, len(t) if n is None else n, t.ctypes.data if ptr is None else ptr, flags))

    good_t = rows["spheres"]
    refused = {"goals: an unknown binding": lambda: set_goals([(1, 0, 0, 0, (0, 0, 1), 0)], binding=99), "goals: more than 16": lambda: set_goals([(1, 0, 0, 0, (0, 0, 1), 0)] * 17),
               "goals: null": lambda: set_goals([(1, 0, 0, 0, (0, 0, 1), 0)], null=True),
               "targets: an unknown binding": lambda: set_targets(good_t, binding=99), "targets: another count": lambda: set_targets(good_t[:1]),
               "targets: null": lambda: set_targets(good_t, ptr=0), "targets: unknown flag bits": lambda: set_targets(good_t, flags=2),
               "targets: host memory given as device memory": lambda: set_targets(good_t, flags=frt.GOAL_TARGETS_DEVICE),
               "targets: a device tensor of another shape": lambda: r.set_rig_goal_targets(mesh, torch.zeros((2, 7), device=f"cuda:{r.device}")),
               "targets: a device tensor of another count": lambda: r.set_rig_goal_targets(mesh, torch.zeros((3, 8), device=f"cuda:{r.device}"))}
    for what, table in bad_goals(rigs["spheres"].num_nodes, limb).items():
        refused["goals: " + what] = lambda table=table: set_goals(table)
    for what, t in bad_targets(good_t).items():      # (goal 1 of the binding is an aim)
        refused["targets: " + what] = lambda t=t: set_targets(t)
    for what, call in refused.items():
        with pytest.raises(frt.FrtError):
            call()
            pytest.fail(f"not refused: {what}")
        assert (r.transform_rejects(), r.deform_rejects()) == counters, what
    assert _scene(r) == start
    r.animate_layers(mesh, layers)      # the binding's goals and targets are the ones it had
    again = r.read_rig_pose(mesh)
    assert bits(again[0]) == bits(pose[0]) and bits(again[1]) == bits(pose[1]) and _scene(r) == start
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); twin.render(cam)
    assert r.read_accum().tobytes() == twin.read_accum().tobytes()
    r.render_phases(cam, frt.PHASE_GBUFFER)      # inside an open frame
    with pytest.raises(frt.FrtError, match="error -4"):
        set_targets(good_t)
    with pytest.raises(frt.FrtError, match="error -4"):
        set_goals([(1, 0, 0, 0, (0, 0, 1), 0)])
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert _scene(r) == start and (r.transform_rejects(), r.deform_rejects()) == counters


def test_multi_renderer(gpu):
    """Two strips on one device: the frame equals that of a single renderer under the same goals on the device."""
    frt = gpu
    desc, rig, fs, meshes = _character(frt)
    goals = to_goals(frt, _limb(desc))
    rows = targets_for(_limb(desc), np.random.default_rng(2), 0.3)
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
