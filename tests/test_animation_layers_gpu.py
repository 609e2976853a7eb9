"""Layering clips on the device (include/frt.h: frt_renderer_set_rig_masks, _animate_layers, _animate_instances_layers, _animate_cast_layers; DESIGN.md
section 11, "Layering clips"): the kernels' palette, weights and matrices are frt_rig_evaluate_layers' and frt_rig_evaluate_nodes_layers', bit for
bit, on the rig shapes at which they could go wrong, for 1, 2 and 8 layers, every mode, no masks, 0 / 1 masks and fractional ones, tight and fully
random rotations; masks set between two animate calls act in stream order; a layered cast leaves what the single layered calls leave, each binding
under its own masks, and rejects a half as a whole; after animate_layers the replica equals the host scene after SceneBuilder.animate_layers and a
frame equals that of a renderer created from it; what is refused enqueues nothing; a MultiRenderer's strips follow; and the single-clip and blend
calls made after layered ones still give their host bits. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_skin_gpu import check_replica, W, H
from test_animation_nodes_gpu import EVERY as SCENE      # (with the instance records and the lights)
from test_animation_gpu import SHAPES, SPARE, CHARACTER, bind_synthetic
from test_animation_blend_gpu import character_blend_rig, near_identity
from test_mesh_deform import PLANE
from _skin_model import F, scene_with_a_spare_mesh
from _cast_scene import burst_clip
from _blend_model import make_blend_rig, random_blends
from _layers_model import L, MODES, to_layers, random_masks, random_stacks

pytestmark = pytest.mark.gpu
LAYER_COUNTS = (1, 2, 8)
INSTANCE_COUNTS = (1, 257)      # one lane; past the 256-lane stride of the kernel's last phase
MASK_KINDS = (None, "binary", "fractional")


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def _scene(r):
    return {w: r.read_scene(w).tobytes() for w in SCENE}


def stacks_of(desc, nmasks, seed=0):
    """For 1, 2 and 8 layers: one stack of every mode and one of the three mixed (one layer: the base alone)."""
    out = random_stacks(desc, 1, 1, "blend", seed=seed)
    for nl in LAYER_COUNTS[1:]:
        for mode in MODES + ("mixed",):
            out += random_stacks(desc, nl, 1, mode, nmasks=nmasks, seed=seed)
    return out


@pytest.mark.parametrize("which", list(SHAPES))
def test_palette_and_weights_have_the_host_bits(gpu, which):
    frt = gpu
    shape, joints, targets = SHAPES[which]
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    for spread in (0.5, None):      # rotations close together, then fully random ones (the short way round flips signs)
        desc = make_blend_rig(shape, nclips=3, joints=joints, num_targets=targets, keys=(1, 2, 33), spread=spread)
        rig = frt.Rig(**desc)
        bind_synthetic(frt, r, meshes, [SPARE], rig)
        b = r.bind_rig(rig, [SPARE])
        for kind in MASK_KINDS:
            masks = None if kind is None else random_masks(desc, 4, seed=3, kind=kind)
            r.set_rig_masks(b, masks)
            for rows in stacks_of(desc, 0 if kind is None else 4):
                layers = to_layers(frt, rows)
                r.animate_layers(b, layers)
                got, want = r.read_rig_pose(b), rig.evaluate_layers(layers, masks)
                assert bits(got[0]) == bits(want[0]), f"{which}, spread {spread}, masks {kind}: palette under {rows}"
                assert bits(got[1]) == bits(want[1]), f"{which}, spread {spread}, masks {kind}: weights under {rows}"
        r.unbind_rig(b)
    assert r.deform_rejects() == 0


@pytest.mark.parametrize("n", INSTANCE_COUNTS)
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
        desc = make_blend_rig(shape, nclips=3, joints="none", num_targets=0, keys=(1, 2, 33), spread=None if shape == "tree257" else 0.5)
        rig = frt.Rig(**desc, nodes_only=True)
        nodes = rng.integers(0, rig.num_nodes, n)
        masks = random_masks(desc, 4, seed=n)
        for kw in ({}, {"root": near_identity(rng, 1)[0], "offsets": near_identity(rng, n)}):
            b = r.bind_rig_instances(rig, ids, nodes, **kw)
            r.set_rig_masks(b, masks)
            for rows in stacks_of(desc, 4, seed=1):
                layers = to_layers(frt, rows)
                r.animate_instances_layers(b, layers)
                assert bits(r.read_rig_instances(b)) == bits(rig.evaluate_nodes_layers(layers, nodes, masks=masks, **kw)), f"{shape}, n {n}, {sorted(kw)}: {rows}"
            r.unbind_rig(b)
    assert r.transform_rejects() == 0


def test_masks_act_in_stream_order(gpu):
    """bind, set_rig_masks, animate, set_rig_masks with other masks (and another count), animate, with no wait in between: the replica after the
    second call is the host scene posed under the second masks, and a twin that only ever saw the first masks shows the first call's bits."""
    frt = gpu
    desc = character_blend_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r, twin = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    for x in (r, twin, fs):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    first, second = random_masks(desc, 2, seed=1), random_masks(desc, 3, seed=2, kind="binary")
    one = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.8, mask=1, mode="override"), frt.Layer("c2", 0.6, 0.7, mask=0, mode="additive", reference=("c2", 0.3))]
    two = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.8, mask=2, mode="override"), frt.Layer("c2", 0.6, 0.7, mask=0, mode="additive", reference=("c2", 0.3))]
    b = r.bind_rig(rig, CHARACTER)
    r.set_rig_masks(b, first)
    r.animate_layers(b, one)
    r.set_rig_masks(b, second)
    r.animate_layers(b, two)
    got, want = r.read_rig_pose(b), rig.evaluate_layers(two, second)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    assert bits(want[0]) != bits(rig.evaluate_layers(one, first)[0]) and bits(want[0]) != bits(rig.evaluate_layers(one, second[:2])[0])
    fs.animate_layers(rig, CHARACTER, one, first)
    fs.animate_layers(rig, CHARACTER, two, second)
    check_replica(frt, r, fs, "two layered calls with a change of masks between them")
    tb = twin.bind_rig(rig, CHARACTER)
    twin.set_rig_masks(tb, first)
    twin.animate_layers(tb, one)
    got, want = twin.read_rig_pose(tb), rig.evaluate_layers(one, first)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    # the same pair once more on one renderer, the first call's pose read between (a read waits): each animate shows its own masks' bits
    r.set_rig_masks(b, first)
    r.animate_layers(b, one)
    r.set_rig_masks(b, second)
    mid = r.read_rig_pose(b)
    assert bits(mid[0]) == bits(want[0]) and bits(mid[1]) == bits(want[1])
    r.set_rig_masks(b, None)      # cleared: a layer that names a mask is refused, a list without masks is taken
    with pytest.raises(frt.FrtError):
        r.animate_layers(b, one)
    r.animate_layers(b, [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")])
    assert r.deform_rejects() == 0


def test_replica_and_frame_equal_the_host_scene(gpu):
    frt = gpu
    desc = character_blend_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam)
    start = r.read_scene("tri_slots").tobytes()
    for x in (r, fs):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b = r.bind_rig(rig, CHARACTER)
    masks = np.stack([rig.mask(3), rig.mask([1, 5], value=0.5, base=0.125)])
    r.set_rig_masks(b, masks)
    for f in (0.0, 0.3, 1.0):      # walk, wave with a limb, lean on top: the override fades in over a subtree, the clips by name
        layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.55, f, mask=0, mode="override", morph=False), frt.Layer("c2", 0.5, 0.5, mask=1, mode="additive", reference=("c2", 0.3))]
        r.animate_layers(b, layers)
        fs.animate_layers(rig, CHARACTER, layers, masks)
        got, want = r.read_rig_pose(b), rig.evaluate_layers(layers, masks)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
        check_replica(frt, r, fs, f"animate_layers at fade {f}")
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    r.clear()
    rf = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)      # from the layered host scene
    r.render(cam); rf.render(cam)
    compare_all(r.read_buffer, rf.read_buffer, 0, "a layered replica vs a renderer created from the layered host scene")


def _cast_world(frt, extra_clips=()):
    """Two renderers over the scene with a spare mesh; two mesh bindings (the spare mesh; the two spheres) and one instance binding (instances 0 and
    1), each with a rig of its own and a mask set of its own (3, 2 and 1 masks)."""
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    descs = {"spare": character_blend_rig(frt, seed=5), "spheres": character_blend_rig(frt, seed=3, extra_clips=extra_clips),
             "props": make_blend_rig("tree12", nclips=3, seed=4, joints="none", num_targets=0, keys=(2, 5), spread=0.2)}
    descs["props"]["translations"] = F(0.05) * descs["props"]["translations"]
    for _, channels in descs["props"]["clips"]:
        for ch in channels:
            if ch["path"] == "translation":
                ch["values"] = F(0.05) * ch["values"]
    rigs = {k: frt.Rig(**d, nodes_only=k == "props") for k, d in descs.items()}
    masks = {"spare": random_masks(descs["spare"], 3, seed=1), "spheres": random_masks(descs["spheres"], 2, seed=2, kind="binary"), "props": random_masks(descs["props"], 1, seed=3)}
    pair = []
    for _ in range(2):
        r = frt.Renderer(fs, W, H, max_depth=2)
        bind_synthetic(frt, r, meshes, [SPARE], rigs["spare"], seed=7)
        bind_synthetic(frt, r, meshes, CHARACTER, rigs["spheres"])
        b = {"spare": r.bind_rig(rigs["spare"], [SPARE]), "spheres": r.bind_rig(rigs["spheres"], CHARACTER), "props": r.bind_rig_instances(rigs["props"], [1, 0], [3, 7])}
        for k in b:
            r.set_rig_masks(b[k], masks[k])
        pair.append((r, b))
    return fs, descs, rigs, masks, pair


def test_a_layered_cast_is_the_single_layered_calls(gpu):
    frt = gpu
    fs, descs, rigs, masks, ((r, b), (other, b2)) = _cast_world(frt)
    assert b == b2
    start = _scene(r)
    for i in range(3):
        rows = {"spheres": random_stacks(descs["spheres"], 8, 1, "mixed", nmasks=2, seed=i)[0], "props": random_stacks(descs["props"], 2, 1, MODES[i], nmasks=1, seed=i)[0],
                "spare": random_stacks(descs["spare"], 1 if i == 0 else 3, 1, "mixed", nmasks=3, seed=i)[0]}
        layers = {k: to_layers(frt, v) for k, v in rows.items()}
        order = ("spheres", "props", "spare") if i != 1 else ("spare", "spheres", "props")      # different layer counts, the kinds in mixed order
        r.animate_cast_layers([(b[k], layers[k]) for k in order])
        other.animate_instances_layers(b["props"], layers["props"])
        other.animate_layers(b["spare"], layers["spare"])
        other.animate_layers(b["spheres"], layers["spheres"])
        got, want = _scene(r), _scene(other)
        for x in SCENE:
            assert got[x] == want[x], f"round {i}: {x}"
        assert got["tri_slots"] != start["tri_slots"]
        for k in ("spare", "spheres"):      # each binding under its own masks
            pose, host = r.read_rig_pose(b[k]), rigs[k].evaluate_layers(layers[k], masks[k])
            assert bits(pose[0]) == bits(host[0]) and bits(pose[1]) == bits(host[1]), f"round {i}: {k}"
        assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_layers(layers["props"], [3, 7], masks=masks["props"])), f"round {i}"
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0) == (other.transform_rejects(), other.deform_rejects())
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); other.render(cam)
    assert r.read_accum().tobytes() == other.read_accum().tobytes()


def test_layers_that_overflow_in_one_character_reject_the_mesh_half_once(gpu):
    frt = gpu
    fs, descs, rigs, masks, ((r, b), (other, _)) = _cast_world(frt, extra_clips=[burst_clip()])
    burst = [("c0", 0.4, 1.0), frt.Layer("burst", 1.0, 8.0, mode="additive")]      # eight times translations of 3e38 of a node and its child
    quiet = [("c0", 0.4, 1.0), frt.Layer("burst", 0.0, 8.0, mode="additive")]
    assert not np.isfinite(rigs["spheres"].evaluate_layers(burst)[0]).all() and np.isfinite(rigs["spheres"].evaluate_layers(quiet)[0]).all()
    calm = {"spare": [("c0", 0.4, 1.0), frt.Layer("c2", 0.5, 1.0, mask=2, mode="override")], "props": [("c1", 0.5, 1.0), frt.Layer("c0", 0.3, 0.5, mask=0)]}
    start = _scene(r)
    r.animate_cast_layers([(b["spare"], calm["spare"]), (b["spheres"], burst), (b["props"], calm["props"])])
    other.animate_instances_layers(b["props"], calm["props"])      # what the call applies: its instance half and nothing else
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 1)
    got, want = _scene(r), _scene(other)
    for x in SCENE:
        assert got[x] == want[x], x
    assert got["instances_dev"] != start["instances_dev"] and got["attributes"] == start["attributes"]
    r.animate_cast_layers([(b["spare"], calm["spare"]), (b["spheres"], quiet), (b["props"], calm["props"])])      # and a clean cast applies
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 1) and _scene(r)["attributes"] != start["attributes"]


def test_refusals_enqueue_nothing(gpu):
    frt = gpu
    from frt._lib import check
    from test_animation_layers import _bad_lists
    lib = frt.lib()
    S, E = frt.ClipLayer, frt.CastLayersEntry
    fs, descs, rigs, masks, ((r, b), (twin, _)) = _cast_world(frt)      # the twin is never handed a refused call
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); twin.render(cam)
    assert r.read_accum().tobytes() == twin.read_accum().tobytes()
    mesh, inst = b["spheres"], b["props"]      # two masks and three clips; one mask and three clips
    r.animate_layers(mesh, [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mask=1, mode="override")])
    twin.animate_layers(mesh, [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mask=1, mode="override")])
    start, counters, pose = _scene(r), (r.transform_rejects(), r.deform_rejects()), r.read_rig_pose(mesh)

    def one(rows, n=None, binding=mesh, flags=0, null=False, instances=False):
        table = (S * max(len(rows), 1))(*[S(*x) for x in rows])
        n = len(rows) if n is None else n
        if instances:
            check(lib.frt_renderer_animate_instances_layers(r._h, binding, n, None if null else table))
        else:
            check(lib.frt_renderer_animate_layers(r._h, binding, n, None if null else table, flags))

    def cast(entries, rows, n=None, nl=None, flags=0, null_entries=False, null_layers=False):
        et = (E * max(len(entries), 1))(*[E(*x) for x in entries])
        st = (S * max(len(rows), 1))(*[S(*x) for x in rows])
        check(lib.frt_renderer_animate_cast_layers(r._h, len(entries) if n is None else n, None if null_entries else et, len(rows) if nl is None else nl,
                                                   None if null_layers else st, flags))

    def set_masks(binding, nmasks, m):
        check(lib.frt_renderer_set_rig_masks(r._h, binding, nmasks, None if m is None else m.ctypes.data))

    g0, g1, add, bad_lists = _bad_lists(3)
    good = [g0, g1]
    ents = [(mesh, 0, 2, 0), (inst, 0, 1, 0)]
    twelve = rigs["spheres"].num_nodes
    ok_masks = np.full((2, twelve), 0.5, F)
    refused = {"n == 0": lambda: one(good, n=0), "n > 8": lambda: one(good * 5, n=9), "null layers": lambda: one(good, null=True),
               "unknown flag bits": lambda: one(good, flags=4), "an unknown binding": lambda: one(good, binding=99),
               "an instance binding": lambda: one(good, binding=inst), "a mesh binding": lambda: one(good, binding=mesh, instances=True),
               "instances: n == 0": lambda: one(good, n=0, binding=inst, instances=True), "instances: null layers": lambda: one(good, binding=inst, null=True, instances=True),
               "a clip name the rig does not have": lambda: r.animate_layers(mesh, [("walk", 0.0, 1.0)]),
               "cast: n == 0": lambda: cast(ents, good, n=0), "cast: null entries": lambda: cast(ents, good, null_entries=True),
               "cast: no layers": lambda: cast(ents, good, nl=0), "cast: null layers": lambda: cast(ents, good, null_layers=True),
               "cast: unknown flag bits": lambda: cast(ents, good, flags=4), "cast: reserved != 0": lambda: cast([ents[0], (inst, 0, 1, 1)], good),
               "cast: a range that overruns nlayers": lambda: cast([ents[0], (inst, 1, 2, 0)], good),
               "cast: a range that begins behind nlayers": lambda: cast([ents[0], (inst, 2, 1, 0)], good),
               "cast: a range that wraps": lambda: cast([ents[0], (inst, 0xFFFFFFFF, 2, 0)], good),
               "cast: an empty range": lambda: cast([ents[0], (inst, 0, 0, 0)], good), "cast: a range of nine": lambda: cast([(mesh, 0, 9, 0)], good * 5),
               "cast: a binding named twice": lambda: cast(ents + [(mesh, 0, 1, 0)], good), "cast: an unknown binding": lambda: cast([ents[0], (99, 0, 1, 0)], good),
               "cast: a range whose base is an override layer": lambda: cast([ents[0], (inst, 1, 1, 0)], good),
               "masks: an unknown binding": lambda: set_masks(99, 2, ok_masks), "masks: more than 16": lambda: set_masks(mesh, 17, np.zeros((17, twelve), F)),
               "masks: null": lambda: set_masks(mesh, 2, None), "masks: of another rig's size": lambda: r.set_rig_masks(mesh, np.zeros((2, twelve + 1), F))}
    one_of_one = [g0, (1, 0.5, 0.5, 1, 1, 0, 0.0, 0)]      # mask 1: the mesh binding has it, the instance binding, with one mask, does not
    refused["instances: mask 1 of one"] = lambda: one(one_of_one, binding=inst, instances=True)
    refused["cast: mask 1 of the instance binding's one"] = lambda: cast([(mesh, 0, 2, 0), (inst, 0, 2, 0)], one_of_one)
    for what, x in (("NaN", np.nan), ("inf", np.inf), ("negative", -0.5), ("above one", 1.5)):
        m = ok_masks.copy()
        m[1, twelve - 1] = x
        refused["masks: " + what] = lambda m=m: set_masks(mesh, 2, m)
    for what, rows in bad_lists.items():
        refused[what] = lambda rows=rows: one(rows)
        refused["instances: " + what] = lambda rows=rows: one(rows, binding=inst, instances=True)
        refused["cast: " + what] = lambda rows=rows: cast([(inst, 0, 1, 0), (mesh, 1, 2, 0)], [g0] + rows)
    for what, call in refused.items():
        with pytest.raises(frt.FrtError):
            call()
            pytest.fail(f"not refused: {what}")
        assert (r.transform_rejects(), r.deform_rejects()) == counters, what
    assert _scene(r) == start
    again = r.read_rig_pose(mesh)      # the binding's masks are the ones it had: the same call gives the same bits
    assert bits(again[0]) == bits(pose[0]) and bits(again[1]) == bits(pose[1])
    r.animate_layers(mesh, [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mask=1, mode="override")])
    again = r.read_rig_pose(mesh)
    assert bits(again[0]) == bits(pose[0]) and bits(again[1]) == bits(pose[1]) and _scene(r) == start
    cam = frt.CameraController().build_uniform(W / H, 1, fs.num_lights)      # nothing was enqueued: the next frame is the twin's
    r.render(cam); twin.render(cam)
    assert r.read_accum().tobytes() == twin.read_accum().tobytes()
    r.render_phases(cam, frt.PHASE_GBUFFER)      # inside an open frame
    with pytest.raises(frt.FrtError, match="error -4"):
        one(good)
    with pytest.raises(frt.FrtError, match="error -4"):
        cast(ents, good)
    with pytest.raises(frt.FrtError, match="error -4"):
        set_masks(mesh, 2, ok_masks)
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert _scene(r) == start and (r.transform_rejects(), r.deform_rejects()) == counters
    cast(ents, good, flags=frt.DEFORM_RECOMPUTE_NORMALS)      # and the good calls apply
    one(good); one([g0, (1, 0.5, 0.5, 0, 2, 2, 0.25, 1)], binding=inst, instances=True)
    assert _scene(r)["tri_slots"] != start["tri_slots"] and (r.transform_rejects(), r.deform_rejects()) == counters


def test_multi_renderer(gpu):
    """Two strips on one device: every strip's rows of the frame equal those of a single renderer layered on the device."""
    frt = gpu
    desc = character_blend_rig(frt)
    rig = frt.Rig(**desc)
    props = make_blend_rig("tree12", nclips=2, seed=4, joints="none", num_targets=0, keys=(2, 5), spread=0.2)
    props["translations"] = F(0.05) * props["translations"]
    for _, channels in props["clips"]:
        for ch in channels:
            if ch["path"] == "translation":
                ch["values"] = F(0.05) * ch["values"]
    prig = frt.Rig(**props, nodes_only=True)
    masks, pmasks = random_masks(desc, 2, seed=4), prig.mask(3, value=0.75)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b, bi = one.bind_rig(rig, CHARACTER), one.bind_rig_instances(prig, [1, 0], [3, 7])
    one.set_rig_masks(b, masks); one.set_rig_masks(bi, pmasks)
    for step, f in enumerate((0.25, 0.7)):
        layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, f, mask=1, mode="override"), frt.Layer("c2", 0.6, 0.5, mask=0, mode="additive")]
        moves = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, f, mask=0)]
        if step == 0:
            multi.animate_layers(rig, CHARACTER, layers, masks)
            multi.animate_instances_layers(prig, [1, 0], [3, 7], moves, pmasks)
            one.animate_instances_layers(bi, moves)
            one.animate_layers(b, layers)
        else:
            multi.animate_cast_layers([(rig, CHARACTER, layers, masks), (prig, [1, 0], [3, 7], moves, pmasks)])
            one.animate_cast_layers([(b, layers), (bi, moves)])
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), f


def test_single_clip_and_blend_calls_after_layered_ones_keep_their_bits(gpu):
    """The instantiations are separate: a layered call leaves nothing behind that a single-clip or a blend call of the same binding would see."""
    frt = gpu
    fs, descs, rigs, masks, ((r, b), _) = _cast_world(frt)
    rig, desc = rigs["spheres"], descs["spheres"]
    layers = to_layers(frt, random_stacks(desc, 8, 1, "mixed", nmasks=2, seed=5)[0])
    r.animate_layers(b["spheres"], layers)
    r.animate_cast_layers([(b["props"], [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mask=0, mode="additive")]), (b["spare"], [("c1", 0.5, 1.0)])])
    r.animate(b["spheres"], "c1", 0.5)
    got, want = r.read_rig_pose(b["spheres"]), rig.evaluate("c1", 0.5)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    rows = random_blends(desc, 3, 1, seed=2)[0]
    r.animate_blend(b["spheres"], rows)
    got, want = r.read_rig_pose(b["spheres"]), rig.evaluate_blend(rows)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    r.animate_instances(b["props"], "c2", 0.45)
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes("c2", 0.45, [3, 7]))
    moves = random_blends(descs["props"], 2, 1, seed=3)[0]
    r.animate_cast_blend([(b["props"], moves), (b["spare"], random_blends(descs["spare"], 2, 1, seed=4)[0])])
    assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_blend(moves, [3, 7]))
    r.animate_layers(b["spheres"], layers)      # and the layered call again, after them
    got, want = r.read_rig_pose(b["spheres"]), rig.evaluate_layers(layers, masks["spheres"])
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0)
