"""Blending clips on the device (include/frt.h: frt_renderer_animate_blend, _animate_instances_blend, _animate_cast_blend; DESIGN.md section 11,
"Blending clips"): the kernels' palette, weights and matrices are frt_rig_evaluate_blend's and frt_rig_evaluate_nodes_blend's, bit for bit, on the rig
shapes at which they could go wrong, for 1, 2 and 8 samples, fully random rotations and a zero weight in every place; after animate_blend the replica
equals the host scene after SceneBuilder.animate_blend and a frame equals that of a renderer created from it; a blended cast leaves what the single
blend calls leave and rejects a half as a whole; what is refused enqueues nothing; a MultiRenderer's strips follow. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_skin_gpu import check_replica, _replica, EVERY, W, H
from test_animation_nodes_gpu import EVERY as SCENE      # (with the instance records and the lights)
from test_animation_gpu import SHAPES, SPARE, CHARACTER, bind_synthetic
from test_mesh_deform import PLANE
from _skin_model import F, scene_with_a_spare_mesh
from _cast_scene import burst_clip
from _blend_model import make_blend_rig, random_blends

pytestmark = pytest.mark.gpu
SAMPLE_COUNTS = (1, 2, 8)
INSTANCE_COUNTS = (1, 257)      # one lane; past the 256-lane stride of the kernel's last phase


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def _scene(r):
    return {w: r.read_scene(w).tobytes() for w in SCENE}


def near_identity(rng, n, spread=0.1):
    m = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (spread * rng.standard_normal((n, 9))).astype(F)
    m[:, 12:15] = (spread * rng.standard_normal((n, 3))).astype(F)
    return m


def blends_of(desc, seed=0):
    """For 1, 2 and 8 samples: two blends with every weight positive, and one each with a zero weight in first, middle and last place."""
    out = []
    for ns in SAMPLE_COUNTS:
        out += random_blends(desc, ns, 2, seed=seed)
        if ns > 1:
            for z in (0, ns // 2, -1):
                out += random_blends(desc, ns, 1, seed=seed + 3 + z, zero_at=z)
    return out


def character_blend_rig(frt, seed=3, extra_clips=()):
    """A 12-node rig near the identity with three clips that all have channels (the posed spheres stay about where they were), 3 targets."""
    desc = make_blend_rig("tree12", nclips=3, seed=seed, joints="subset", num_targets=3, keys=(2, 5), spread=0.2)
    desc["translations"] = F(0.1) * desc["translations"]
    desc["rotations"] = np.tile(F([0, 0, 0, 1]), (12, 1))
    for _, channels in desc["clips"]:
        for ch in channels:
            if ch["path"] == "translation":
                ch["values"] = F(0.05) * ch["values"]
            if ch["path"] == "rotation":      # (keys were drawn about the old rest rotation: draw them about the identity)
                v = F([0, 0, 0, 1]) + F(0.1) * ch["values"]
                ch["values"] = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)
                if ch["interpolation"] == "CUBICSPLINE":
                    ch["values"][:, 0::2] = F(0.02) * ch["values"][:, 0::2]
    desc["clips"] = desc["clips"] + list(extra_clips)
    return desc


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
        for rows in blends_of(desc):
            r.animate_blend(b, rows)
            got, want = r.read_rig_pose(b), rig.evaluate_blend(rows)
            assert bits(got[0]) == bits(want[0]), f"{which}, spread {spread}: palette under {rows}"
            assert bits(got[1]) == bits(want[1]), f"{which}, spread {spread}: weights under {rows}"
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
        for kw in ({}, {"root": near_identity(rng, 1)[0], "offsets": near_identity(rng, n)}):
            b = r.bind_rig_instances(rig, ids, nodes, **kw)
            for rows in blends_of(desc, seed=1):
                r.animate_instances_blend(b, rows)
                assert bits(r.read_rig_instances(b)) == bits(rig.evaluate_nodes_blend(rows, nodes, **kw)), f"{shape}, n {n}, {sorted(kw)}: {rows}"
            r.unbind_rig(b)
    assert r.transform_rejects() == 0


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
    for f in (0.0, 0.3, 1.0):      # a cross-fade from "c0" to "c1", the clips by name
        rows = [("c0", 0.4, 1.0 - f), ("c1", 0.55, f)]
        r.animate_blend(b, rows)
        fs.animate_blend(rig, CHARACTER, rows)
        got, want = r.read_rig_pose(b), rig.evaluate_blend(rows)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
        check_replica(frt, r, fs, f"animate_blend at fade {f}")
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    r.clear()
    rf = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)      # from the blended host scene
    r.render(cam); rf.render(cam)
    compare_all(r.read_buffer, rf.read_buffer, 0, "a blended replica vs a renderer created from the blended host scene")


def _cast_world(frt, extra_clips=()):
    """Two renderers over the scene with a spare mesh; two mesh bindings (the spare mesh; the two spheres) and one instance binding (instances 0 and
    1), each with a rig of its own."""
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    descs = {"spare": character_blend_rig(frt, seed=5), "spheres": character_blend_rig(frt, seed=3, extra_clips=extra_clips),
             "props": make_blend_rig("tree12", nclips=3, seed=4, joints="none", num_targets=0, keys=(2, 5), spread=0.2)}
    descs["props"]["translations"] = F(0.05) * descs["props"]["translations"]
    for _, channels in descs["props"]["clips"]:
        for ch in channels:
            if ch["path"] == "translation":
                ch["values"] = F(0.05) * ch["values"]
    rigs = {k: frt.Rig(**d, nodes_only=k == "props") for k, d in descs.items()}
    pair = []
    for _ in range(2):
        r = frt.Renderer(fs, W, H, max_depth=2)
        bind_synthetic(frt, r, meshes, [SPARE], rigs["spare"], seed=7)
        bind_synthetic(frt, r, meshes, CHARACTER, rigs["spheres"])
        b = {"spare": r.bind_rig(rigs["spare"], [SPARE]), "spheres": r.bind_rig(rigs["spheres"], CHARACTER), "props": r.bind_rig_instances(rigs["props"], [1, 0], [3, 7])}
        pair.append((r, b))
    return fs, descs, rigs, pair


def test_a_blended_cast_is_the_single_blend_calls(gpu):
    frt = gpu
    fs, descs, rigs, ((r, b), (other, b2)) = _cast_world(frt)
    assert b == b2
    start = _scene(r)
    for i in range(3):
        rows = {"spheres": random_blends(descs["spheres"], 8, 1, seed=i)[0], "props": random_blends(descs["props"], 2, 1, seed=i, zero_at=i if i < 2 else None)[0],
                "spare": random_blends(descs["spare"], 1 if i == 0 else 3, 1, seed=i)[0]}
        order = ("spheres", "props", "spare") if i != 1 else ("spare", "spheres", "props")      # different sample counts, the kinds in mixed order
        r.animate_cast_blend([(b[k], rows[k]) for k in order])
        other.animate_instances_blend(b["props"], rows["props"])
        other.animate_blend(b["spare"], rows["spare"])
        other.animate_blend(b["spheres"], rows["spheres"])
        got, want = _scene(r), _scene(other)
        for x in SCENE:
            assert got[x] == want[x], f"round {i}: {x}"
        assert got["tri_slots"] != start["tri_slots"]
        for k in ("spare", "spheres"):
            pose, host = r.read_rig_pose(b[k]), rigs[k].evaluate_blend(rows[k])
            assert bits(pose[0]) == bits(host[0]) and bits(pose[1]) == bits(host[1]), f"round {i}: {k}"
        assert bits(r.read_rig_instances(b["props"])) == bits(rigs["props"].evaluate_nodes_blend(rows["props"], [3, 7])), f"round {i}"
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 0) == (other.transform_rejects(), other.deform_rejects())
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); other.render(cam)
    assert r.read_accum().tobytes() == other.read_accum().tobytes()


def test_a_blend_that_overflows_in_one_character_rejects_the_mesh_half_once(gpu):
    frt = gpu
    fs, descs, rigs, ((r, b), (other, _)) = _cast_world(frt, extra_clips=[burst_clip()])
    burst = [("c0", 0.4, 1.0), ("burst", 1.0, 1e30)]      # all of the weight, in float32, on translations of 3e38 of a node and its child
    assert not np.isfinite(rigs["spheres"].evaluate_blend(burst)[0]).all() and np.isfinite(rigs["spheres"].evaluate_blend([("c0", 0.4, 1.0), ("burst", 0.0, 1.0)])[0]).all()
    calm = {"spare": [("c0", 0.4, 1.0), ("c2", 0.5, 2.0)], "props": [("c1", 0.5, 1.0), ("c0", 0.3, 0.5)]}
    start = _scene(r)
    r.animate_cast_blend([(b["spare"], calm["spare"]), (b["spheres"], burst), (b["props"], calm["props"])])
    other.animate_instances_blend(b["props"], calm["props"])      # what the call applies: its instance half and nothing else
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 1)
    got, want = _scene(r), _scene(other)
    for x in SCENE:
        assert got[x] == want[x], x
    assert got["instances_dev"] != start["instances_dev"] and got["attributes"] == start["attributes"]
    r.animate_cast_blend([(b["spare"], calm["spare"]), (b["spheres"], [("c0", 0.4, 1.0), ("burst", 0.0, 1.0)]), (b["props"], calm["props"])])      # and a clean cast applies
    assert (r.transform_rejects(), r.deform_rejects()) == (0, 1) and _scene(r)["attributes"] != start["attributes"]


def test_refusals_enqueue_nothing(gpu):
    frt = gpu
    from frt._lib import check
    L = frt.lib()
    S, E = frt.ClipSample, frt.CastBlendEntry
    fs, descs, rigs, ((r, b), (twin, _)) = _cast_world(frt)      # the twin is never handed a refused call
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam); twin.render(cam)
    assert r.read_accum().tobytes() == twin.read_accum().tobytes()
    start, counters = _scene(r), (r.transform_rejects(), r.deform_rejects())
    mesh, inst = b["spheres"], b["props"]

    def one(rows, n=None, binding=mesh, flags=0, null=False, instances=False):
        table = (S * max(len(rows), 1))(*[S(*x) for x in rows])
        n = len(rows) if n is None else n
        if instances:
            check(L.frt_renderer_animate_instances_blend(r._h, binding, n, None if null else table))
        else:
            check(L.frt_renderer_animate_blend(r._h, binding, n, None if null else table, flags))

    def cast(entries, rows, n=None, ns=None, flags=0, null_entries=False, null_samples=False):
        et = (E * max(len(entries), 1))(*[E(*x) for x in entries])
        st = (S * max(len(rows), 1))(*[S(*x) for x in rows])
        check(L.frt_renderer_animate_cast_blend(r._h, len(entries) if n is None else n, None if null_entries else et, len(rows) if ns is None else ns,
                                                None if null_samples else st, flags))

    good = [(0, 0.4, 1.0, 0), (1, 0.5, 2.0, 0)]
    ents = [(mesh, 0, 2, 0), (inst, 1, 1, 0)]
    bad_lists = {"reserved != 0": [good[0], (1, 0.5, 2.0, 1)], "a clip out of range": [good[0], (3, 0.5, 2.0, 0)], "time NaN": [(0, np.nan, 1.0, 0), good[1]],
                 "time inf": [good[0], (1, np.inf, 2.0, 0)], "weight NaN": [good[0], (1, 0.5, np.nan, 0)], "weight inf": [good[0], (1, 0.5, np.inf, 0)],
                 "a negative weight": [good[0], (1, 0.5, -1.0, 0)], "no positive weight": [(0, 0.4, 0.0, 0), (1, 0.5, 0.0, 0)]}
    refused = {"n == 0": lambda: one(good, n=0), "n > 8": lambda: one(good * 5, n=9), "null samples": lambda: one(good, null=True),
               "unknown flag bits": lambda: one(good, flags=4), "an unknown binding": lambda: one(good, binding=99),
               "an instance binding": lambda: one(good, binding=inst), "a mesh binding": lambda: one(good, binding=mesh, instances=True),
               "instances: n == 0": lambda: one(good, n=0, binding=inst, instances=True), "instances: null samples": lambda: one(good, binding=inst, null=True, instances=True),
               "a clip name the rig does not have": lambda: r.animate_blend(mesh, [("walk", 0.0, 1.0)]),
               "cast: n == 0": lambda: cast(ents, good, n=0), "cast: null entries": lambda: cast(ents, good, null_entries=True),
               "cast: no samples": lambda: cast(ents, good, ns=0), "cast: null samples": lambda: cast(ents, good, null_samples=True),
               "cast: unknown flag bits": lambda: cast(ents, good, flags=4), "cast: reserved != 0": lambda: cast([ents[0], (inst, 1, 1, 1)], good),
               "cast: a range that overruns nsamples": lambda: cast([ents[0], (inst, 1, 2, 0)], good),
               "cast: a range that begins behind nsamples": lambda: cast([ents[0], (inst, 2, 1, 0)], good),
               "cast: a range that wraps": lambda: cast([ents[0], (inst, 0xFFFFFFFF, 2, 0)], good),
               "cast: an empty range": lambda: cast([ents[0], (inst, 1, 0, 0)], good), "cast: a range of nine": lambda: cast([(mesh, 0, 9, 0)], good * 5),
               "cast: a binding named twice": lambda: cast(ents + [(mesh, 0, 1, 0)], good), "cast: an unknown binding": lambda: cast([ents[0], (99, 1, 1, 0)], good)}
    for what, rows in bad_lists.items():
        refused[what] = lambda rows=rows: one(rows)
        refused["instances: " + what] = lambda rows=rows: one(rows, binding=inst, instances=True)
        refused["cast: " + what] = lambda rows=rows: cast([(inst, 0, 1, 0), (mesh, 1, 2, 0)], [good[0]] + rows)
    for what, call in refused.items():
        with pytest.raises(frt.FrtError):
            call()
        assert (r.transform_rejects(), r.deform_rejects()) == counters, what
    assert _scene(r) == start
    cam = frt.CameraController().build_uniform(W / H, 1, fs.num_lights)      # nothing was enqueued: the next frame is the twin's
    r.render(cam); twin.render(cam)
    assert r.read_accum().tobytes() == twin.read_accum().tobytes()
    r.render_phases(cam, frt.PHASE_GBUFFER)      # inside an open frame
    with pytest.raises(frt.FrtError, match="error -4"):
        one(good)
    with pytest.raises(frt.FrtError, match="error -4"):
        cast(ents, good)
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert _scene(r) == start and (r.transform_rejects(), r.deform_rejects()) == counters
    cast(ents, good, flags=frt.DEFORM_RECOMPUTE_NORMALS)      # and the good calls apply
    one(good); one(good, binding=inst, instances=True)
    assert _scene(r)["tri_slots"] != start["tri_slots"] and (r.transform_rejects(), r.deform_rejects()) == counters


def test_multi_renderer(gpu):
    """Two strips on one device: every strip's rows of the frame equal those of a single renderer blended on the device."""
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
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b, bi = one.bind_rig(rig, CHARACTER), one.bind_rig_instances(prig, [1, 0], [3, 7])
    for step, f in enumerate((0.25, 0.7)):
        rows, moves = [("c0", 0.4, 1.0 - f), ("c1", 0.5, f), ("c2", 0.6, 0.5)], [("c0", 0.4, f), ("c1", 0.5, 1.0)]
        if step == 0:
            multi.animate_blend(rig, CHARACTER, rows)
            multi.animate_instances_blend(prig, [1, 0], [3, 7], moves)
            one.animate_instances_blend(bi, moves)
            one.animate_blend(b, rows)
        else:
            multi.animate_cast_blend([(rig, CHARACTER, rows), (prig, [1, 0], [3, 7], moves)])
            one.animate_cast_blend([(b, rows), (bi, moves)])
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), f
