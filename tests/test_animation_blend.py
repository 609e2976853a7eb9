"""frt_rig_evaluate_blend and frt_rig_evaluate_nodes_blend, the host specification of blending clips (include/frt.h; DESIGN.md section 11, "Blending
clips"), against tests/_blend_model.py: the identities the contract makes exact, bit for bit; closeness to float64 on random rigs and blends of 2, 3
and 8 samples; the properties that hold under fully random rotations; every refusal, with the outputs untouched; SceneBuilder.animate_blend =
evaluate_blend + set_mesh_poses; the new symbols; and the host forms, stand-alone, under a sanitiser."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from test_mesh_deform import CUBE, SPHERE, EVERYTHING
from test_instance_update import cornell_meshes
from _skin_model import F, make_skin
from _morph_model import make_targets
from _blend_model import make_blend_rig, model_evaluate_blend, random_blends, clip_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Measured on the host (profiles/animation_blend_f64.md): the largest max|f32 - f64| / max|f64| over a palette, over the blends of
# test_random_blends_are_close_to_float64. The host form calls no libm and reproduces exactly; the test asserts twice the measured value.
F64_MEASURED = {"chain1": 6.56e-07, "chain2": 1.22e-06, "chain70": 5.95e-06, "fan65": 1.07e-06, "tree257": 9.15e-07, "tree1024": 1.16e-06}
SAMPLE_COUNTS = (2, 3, 8)


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def same(got, want):
    return [bits(x) for x in got] == [bits(x) for x in want]


def near_identity(rng, n, spread=0.1):
    m = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (spread * rng.standard_normal((n, 9))).astype(F)
    m[:, 12:15] = (spread * rng.standard_normal((n, 3))).astype(F)
    return m


def test_one_sample_and_zero_weights_are_the_single_clip_bit_for_bit(frt):
    desc = make_blend_rig("tree257", nclips=3, seed=1, joints="subset")
    rig = frt.Rig(**desc)
    rng = np.random.default_rng(2)
    nodes = rng.integers(0, rig.num_nodes, 40)
    node_kw = ({}, {"root": near_identity(rng, 1)[0], "offsets": near_identity(rng, 40)})
    times = [clip_times(desc, c, 6, rng) for c in range(3)]
    for i in range(6):
        (ta, tb, tc) = (float(times[c][i]) for c in range(3))
        for clip, t in ((0, ta), (1, tb), (2, tc)):
            want = rig.evaluate(clip, t)
            for w in (1.0, 0.25, 3.0):      # one sample of any positive weight
                assert same(rig.evaluate_blend([(clip, t, w)]), want), (clip, t, w)
            for kw in node_kw:
                assert bits(rig.evaluate_nodes_blend([(clip, t, 0.25)], nodes, **kw)) == bits(rig.evaluate_nodes(clip, t, nodes, **kw))
        # a zero weight in first, middle and last place, and every other sample zero
        a, b = rig.evaluate(0, ta), rig.evaluate(1, tb)
        assert same(rig.evaluate_blend([(0, ta, 2.0), (1, tb, 0.0)]), a)
        assert same(rig.evaluate_blend([(0, ta, 0.0), (1, tb, 0.5)]), b)
        assert same(rig.evaluate_blend([("c2", tc, 0.0), ("c0", ta, 1.0), ("c1", tb, 0.0)]), a)
        assert same(rig.evaluate_blend([(2, tc, 0.0)] * 7 + [(1, tb, 1e-3)]), b)      # eight samples are accepted
        two = [(0, ta, 0.75), (2, tc, 1.5)]
        want = rig.evaluate_blend(two)
        assert not same(want, a) and not same(want, rig.evaluate(2, tc))
        for at in range(3):      # zero-weight samples anywhere in the list change nothing
            rows = list(two)
            rows.insert(at, (1, tb, 0.0))
            assert same(rig.evaluate_blend(rows), want), at
            for kw in node_kw:
                assert bits(rig.evaluate_nodes_blend(rows, nodes, **kw)) == bits(rig.evaluate_nodes_blend(two, nodes, **kw))
        for kw in node_kw:
            assert bits(rig.evaluate_nodes_blend([(0, ta, 0.0), (1, tb, 3.0)], nodes, **kw)) == bits(rig.evaluate_nodes(1, tb, nodes, **kw))
            assert bits(rig.evaluate_nodes_blend([(0, ta, 3.0), (1, tb, 0.0)], nodes, **kw)) == bits(rig.evaluate_nodes(0, ta, nodes, **kw))
    full = rig.evaluate_blend([(i % 3, float(times[i % 3][i % 6]), 0.5 + i) for i in range(frt.MAX_BLEND_SAMPLES)])
    assert np.isfinite(full[0]).all() and np.isfinite(full[1]).all()


def test_the_split_local_matrix_and_the_defaults_of_a_clip_without_a_weights_channel(frt):
    """The last clip of make_blend_rig has no weights channel: its share of a blend is the default weights."""
    desc = make_blend_rig("chain2", nclips=2, joints="none", num_targets=5)
    rig = frt.Rig(**desc)
    _, w0 = rig.evaluate(0, 0.4)
    _, w1 = rig.evaluate(1, 0.4)
    assert bits(w1) == bits(desc["default_weights"]) and bits(w0) != bits(w1)
    _, w = rig.evaluate_blend([(0, 0.4, 1.0), (1, 0.4, 3.0)])      # a = 0.75, exact
    want = w0.astype(np.float64) * 0.25 + w1.astype(np.float64) * 0.75
    assert np.abs(w - want).max() <= 2.0 ** -23


@pytest.mark.parametrize("shape", list(F64_MEASURED))
def test_random_blends_are_close_to_float64(frt, shape):
    """Rotations within 0.5 rad of the rest rotation: no slerp of a blend is near its sign decision, and no blend is left out."""
    desc = make_blend_rig(shape, nclips=3)
    rig = frt.Rig(**desc)
    n = rig.num_nodes
    met, worst, worst_w = {}, 0.0, 0.0
    for ns in SAMPLE_COUNTS:
        for rows in random_blends(desc, ns, max(3, min(24, 6000 // (n * ns)))):
            pal, w = rig.evaluate_blend(rows)
            mp, mw = model_evaluate_blend(desc, rows, met)
            worst = max(worst, float(np.abs(pal - mp).max() / np.abs(mp).max()))
            worst_w = max(worst_w, float(np.abs(w - mw).max()))
    print(f"{shape}: max |f32 - f64| / max |f64| = {worst:.3e}; weights: {worst_w:.3e}; smallest |d| of a blend's slerp: {met.get('min_abs_d', 1.0):.3f}")
    assert met.get("min_abs_d", 1.0) > 0.5
    assert worst <= 2 * F64_MEASURED[shape]
    # weights of size one: the sampler's 8 x 2^-24 (test_animation.py), carried through a convex mix, and per blended sample at most four more roundings
    # of that size (1 - a, two products, one sum; the rounding of a itself counts for less than |x - r| <= 1 of one)
    assert worst_w <= (8 + 4 * (max(SAMPLE_COUNTS) - 1)) * 2.0 ** -24


def test_fully_random_rotations_keep_the_properties(frt):
    desc = make_blend_rig("tree257", nclips=3, seed=3, spread=None)
    rig = frt.Rig(**desc)
    met = {}
    for ns in SAMPLE_COUNTS:
        for rows in random_blends(desc, ns, 6, seed=5):
            pal, w = rig.evaluate_blend(rows)
            assert np.isfinite(pal).all() and np.isfinite(w).all()
            model_evaluate_blend(desc, rows[:2], met)
            (ca, ta, _), (cb, tb, _) = rows[:2]
            assert same(rig.evaluate_blend([(ca, ta, 1.0), (cb, tb, 0.0)]), rig.evaluate(ca, ta))
            assert same(rig.evaluate_blend([(ca, ta, 0.0), (cb, tb, 1.0)]), rig.evaluate(cb, tb))
    assert met["min_abs_d"] < 0.05      # these blends do meet rotations about a right angle apart in 4-space, either side of the sign decision


def test_refusals_leave_the_outputs_untouched(frt):
    L = frt.lib()
    desc = make_blend_rig("chain2", nclips=2)
    rig = frt.Rig(**desc)
    S = frt.ClipSample
    good = [(0, 0.5, 1.0, 0), (1, 0.5, 2.0, 0)]
    bad = {"n == 0": (0, good), "n > 8": (9, good * 5), "reserved != 0": (2, [good[0], (1, 0.5, 2.0, 1)]), "a clip out of range": (2, [good[0], (2, 0.5, 2.0, 0)]),
           "time NaN": (2, [(0, np.nan, 1.0, 0), good[1]]), "time inf": (2, [good[0], (1, np.inf, 2.0, 0)]), "time -inf": (2, [good[0], (1, -np.inf, 2.0, 0)]),
           "weight NaN": (2, [good[0], (1, 0.5, np.nan, 0)]), "weight inf": (2, [(0, 0.5, np.inf, 0), good[1]]), "a negative weight": (2, [good[0], (1, 0.5, -1.0, 0)]),
           "a negative weight of weight zero's size": (2, [good[0], (1, 0.5, -1e-30, 0)]), "no positive weight": (2, [(0, 0.5, 0.0, 0), (1, 0.5, 0.0, 0)]),
           "a bad clip under a zero weight": (2, [good[0], (7, 0.5, 0.0, 0)])}
    nodes = np.array([1, 0, 1], np.uint32)
    for what, (n, rows) in bad.items():
        table = (S * len(rows))(*[S(*r) for r in rows])
        pal, w, mats = np.full((2, 16), 7.0, F), np.full(3, 7.0, F), np.full((3, 16), 7.0, F)
        assert L.frt_rig_evaluate_blend(rig._h, n, table, pal.ctypes.data, w.ctypes.data) == -1, what
        assert b"rig_evaluate_blend" in L.frt_last_error()
        assert L.frt_rig_evaluate_nodes_blend(rig._h, n, table, 3, nodes.ctypes.data, None, None, mats.ctypes.data) == -1, what
        assert (pal == 7.0).all() and (w == 7.0).all() and (mats == 7.0).all(), what
    table = (S * 2)(*[S(*r) for r in good])
    pal, w, mats = np.full((2, 16), 7.0, F), np.full(3, 7.0, F), np.full((3, 16), 7.0, F)
    assert L.frt_rig_evaluate_blend(rig._h, 2, None, pal.ctypes.data, w.ctypes.data) == -1                      # null samples
    assert L.frt_rig_evaluate_blend(None, 2, table, pal.ctypes.data, w.ctypes.data) == -1
    assert L.frt_rig_evaluate_blend(rig._h, 2, table, None, w.ctypes.data) == -1                                # a null output
    assert L.frt_rig_evaluate_nodes_blend(rig._h, 2, None, 3, nodes.ctypes.data, None, None, mats.ctypes.data) == -1
    assert L.frt_rig_evaluate_nodes_blend(rig._h, 2, table, 0, nodes.ctypes.data, None, None, mats.ctypes.data) == -1
    assert L.frt_rig_evaluate_nodes_blend(rig._h, 2, table, 3, None, None, None, mats.ctypes.data) == -1
    far = np.array([1, 2, 0], np.uint32)                                                                        # a node that is not a node
    assert L.frt_rig_evaluate_nodes_blend(rig._h, 2, table, 3, far.ctypes.data, None, None, mats.ctypes.data) == -1
    root = np.full(16, np.nan, F)
    assert L.frt_rig_evaluate_nodes_blend(rig._h, 2, table, 3, nodes.ctypes.data, root.ctypes.data, None, mats.ctypes.data) == -1
    assert (pal == 7.0).all() and (w == 7.0).all() and (mats == 7.0).all()
    assert L.frt_rig_evaluate_blend(rig._h, 2, table, pal.ctypes.data, w.ctypes.data) == 0 and not (pal == 7.0).any()      # and the good call writes
    for rows in ([("walk", 0.0, 1.0)], [(0, 0.0)], [(0, 0.0, 1.0, 0)], []):
        with pytest.raises(frt.FrtError):
            rig.evaluate_blend(rows)


def test_scene_animate_blend_is_evaluate_blend_then_set_mesh_poses(frt):
    meshes = cornell_meshes(frt)
    ids = [CUBE, SPHERE]
    desc = make_blend_rig("tree257", nclips=3, seed=2, joints="subset", num_targets=4)
    rig = frt.Rig(**desc)
    a, b = frt.scenes.create_cornell_box(), frt.scenes.create_cornell_box()
    before = a.get("tri_slots").tobytes()
    for s in (a, b):
        for m in ids:
            n = len(meshes[m].positions)
            s.set_mesh_morph_targets(m, 0.1 * make_targets(n, rig.num_targets, seed=m))
            s.set_mesh_skin(m, *make_skin(n, rig.num_joints, seed=m), num_joints=rig.num_joints)
    for rows in random_blends(desc, 3, 3, seed=9):
        rows = [(f"c{c}", t, w) for c, t, w in rows]      # clips by name
        a.animate_blend(rig, ids, rows)
        b.set_mesh_poses(ids, *rig.evaluate_blend(rows))
        for w in EVERYTHING:
            assert a.get(w).tobytes() == b.get(w).tobytes(), w
    assert a.get("tri_slots").tobytes() != before
    a.animate_cast_blend([(rig, ids, [("c0", 0.5, 1.0), ("c1", 0.6, 1.0)])], normals="keep")      # a cast of one mesh entry is that call
    b.animate_blend(rig, ids, [("c0", 0.5, 1.0), ("c1", 0.6, 1.0)], normals="keep")
    for w in EVERYTHING:
        assert a.get(w).tobytes() == b.get(w).tobytes(), w
    for bad in ([], [(rig,)], [(rig, ids, [], 1, 2, 3, 4)]):
        with pytest.raises(frt.FrtError):
            a.animate_cast_blend(bad)


def test_symbols_are_exported(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for text in ("#define FRT_MAX_BLEND_SAMPLES 8u", "typedef struct frt_clip_sample { uint32_t clip; float time, weight; uint32_t reserved; } frt_clip_sample;",
                 "typedef struct frt_cast_blend_entry { uint32_t binding, first_sample, num_samples, reserved; } frt_cast_blend_entry;"):
        assert text in header, text
    for name in ("frt_rig_evaluate_blend", "frt_rig_evaluate_nodes_blend", "frt_renderer_animate_blend", "frt_renderer_animate_instances_blend", "frt_renderer_animate_cast_blend"):
        assert hasattr(frt.lib(), name) and name + "(" in header, name
    assert C.sizeof(frt.ClipSample) == 16 and C.sizeof(frt.CastBlendEntry) == 16 and frt.MAX_BLEND_SAMPLES == 8
    for cls in (frt.SceneBuilder, frt.Renderer, frt.MultiRenderer):
        for call in ("animate_blend", "animate_instances_blend", "animate_cast_blend"):
            assert callable(getattr(cls, call)), (cls, call)
    L = frt.lib()
    one = (frt.ClipSample * 1)(frt.ClipSample(0, 0.0, 1.0, 0))
    assert L.frt_renderer_animate_blend(None, 0, 1, one, 0) == -1 and b"animate_blend" in L.frt_last_error()      # a null renderer, before anything else
    assert L.frt_renderer_animate_instances_blend(None, 0, 1, one) == -1
    assert L.frt_renderer_animate_cast_blend(None, 1, (frt.CastBlendEntry * 1)(), 1, one, 0) == -1


def test_host_forms_run_clean_under_a_sanitiser(tmp_path):
    """tools/blend_sanitize.cpp with csrc/frt_animation.cpp, stand-alone, with -fsanitize=address,undefined."""
    exe = str(tmp_path / "blend_sanitize")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math"] + san +
                   [os.path.join(ROOT, "tools", "blend_sanitize.cpp"), os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc", "frt_animation.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok: "), run.stdout + run.stderr
