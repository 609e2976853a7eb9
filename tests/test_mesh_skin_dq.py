"""Dual-quaternion skinning of a built scene, on the host (include/frt.h: frt_scene_set_mesh_skin_ex, FRT_SKIN_DUAL_QUATERNION; DESIGN.md section 11,
"Dual-quaternion skinning"): the new symbols and what they refuse; the old call still binds the linear blend; the defect the mode is for (a ring
under a 170 degree twist); rigid identities; closeness to the float64 model of tests/_skin_dq_model.py with every sigma decision kept clear of its
threshold; the poses that must be refused; batches, rigs and casts that mix the modes; and the host form, stand-alone, under a sanitiser."""
import os
import re
import subprocess
import numpy as np
import pytest
from test_mesh_deform import EVERYTHING
from _skin_model import F, make_skin, make_palette, overflowing_palette
from _skin_dq_model import (D, skin_dq_model, joint_dq, rotation, trs, random_palette, clear_skin, random_weights, ring_mesh, mesh_of, scene_of,
                            posed_positions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frt_scene_set_mesh_skin_ex", "frt_renderer_set_mesh_skin_ex", "frt_multi_renderer_set_mesh_skin_ex")
DQ = "dual_quaternion"
# Measured on the host (profiles/skin_dq_f64.md): per case family of test_close_to_float64 the largest max|f32 - f64| / max|f64| over the posed
# positions of one mesh. The host form calls no libm and reproduces exactly; the test asserts four times the measured value (other seeds: the error
# is a sum of a few dozen roundings). BOUND is the largest of them times 4: what the tests of the defect and of the rigid identities allow.
F64_MEASURED = {"rigid": 1.771e-07, "scaled": 2.874e-07, "one joint": 1.549e-07, "far": 1.597e-07}
BOUND = 4.0 * max(F64_MEASURED.values())
SIGMA_CLEAR = 0.05      # every |dot4(qr_k, qr_pivot)| of the accuracy data is at least this (the model's own margins, asserted)
BRANCH_NEAR = 1e-3      # a Shepperd choice won by less than this could fall the other way in f32: the two candidates must then agree


def test_new_symbols_are_declared_in_the_header(frt):
    text = open(os.path.join(ROOT, "include", "frt.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", text), s
        assert hasattr(frt.lib(), s)
    assert re.search(r"#define FRT_SKIN_DUAL_QUATERNION 1u", text)


def _state(fs):
    return {w: fs.get(w).tobytes() for w in EVERYTHING}


def test_refusals_and_the_old_call(frt):
    lib = frt.lib()
    meshes = [ring_mesh(frt, 12)]
    a, b, c = scene_of(frt, meshes), scene_of(frt, meshes), scene_of(frt, meshes)
    j, w = make_skin(12, 3)
    pal = make_palette(3, 0.4)
    # the old call and _ex with flags 0 bind the same linear skin: the same pose, bit for bit (and the numpy model of the linear blend)
    a.set_mesh_skin(0, j, w, num_joints=3)
    assert lib.frt_scene_set_mesh_skin_ex(b._h, 0, j.ctypes.data, w.ctypes.data, 12, 3, 0) == 0
    c.set_mesh_skin(0, j, w, num_joints=3, mode="linear")
    for s in (a, b, c):
        s.set_mesh_pose(0, pal)
    assert _state(a) == _state(b) == _state(c)
    start = _state(a)
    # an unknown flag bit, with and without the known one, and with null joints: refused, nothing changed (the linear skin is still bound)
    for flags in (2, 3, 0x80000000):
        assert lib.frt_scene_set_mesh_skin_ex(a._h, 0, j.ctypes.data, w.ctypes.data, 12, 3, flags) == -1
        assert b"unknown flag" in lib.frt_last_error()
    assert lib.frt_scene_set_mesh_skin_ex(a._h, 0, None, None, 0, 0, 4) == -1
    for mode in ("dq", "DUAL_QUATERNION", "", None, 1):
        with pytest.raises(frt.FrtError, match="mode must be"):
            a.set_mesh_skin(0, j, w, num_joints=3, mode=mode)
    # the checks of the old call, in its order, through the new one
    assert lib.frt_scene_set_mesh_skin_ex(a._h, 9, j.ctypes.data, w.ctypes.data, 12, 3, 1) == -1
    assert lib.frt_scene_set_mesh_skin_ex(a._h, 0, j.ctypes.data, w.ctypes.data, 11, 3, 1) == -1
    assert lib.frt_scene_set_mesh_skin_ex(a._h, 0, j.ctypes.data, w.ctypes.data, 12, 2, 1) == -1
    unbuilt = frt.SceneBuilder()
    assert lib.frt_scene_set_mesh_skin_ex(unbuilt._h, 0, j.ctypes.data, w.ctypes.data, 12, 3, 1) == -4      # FRT_ERR_STATE: not built
    a.set_mesh_pose(0, pal)
    assert _state(a) == start
    # binding again replaces the mode with the skin, both ways
    a.set_mesh_vertices(0, meshes[0].positions)      # (a bind call takes the positions as they are for its bind pose)
    a.set_mesh_skin(0, j, w, num_joints=3, mode=DQ)
    a.set_mesh_pose(0, pal)
    assert _state(a) != start
    a.set_mesh_vertices(0, meshes[0].positions)
    a.set_mesh_skin(0, j, w, num_joints=3)
    a.set_mesh_pose(0, pal)
    assert _state(a) == start


def _ring_case(frt, angle_deg, mode, n=16, radius=0.5):
    meshes = [ring_mesh(frt, n, radius)]
    fs = scene_of(frt, meshes)
    j = np.tile(np.array([0, 1, 0, 0], np.uint16), (n, 1))
    w = np.tile(F([0.5, 0.5, 0.0, 0.0]), (n, 1))
    fs.set_mesh_skin(0, j, w, num_joints=2, mode=mode)
    pal = np.stack([trs(), trs(rotation([0, 1, 0], np.radians(angle_deg)))])
    fs.set_mesh_pose(0, pal)
    return meshes[0].positions.astype(D), posed_positions(fs, meshes, 0).astype(D), (j, w, pal)


def test_the_defect_and_its_cure(frt):
    """A ring about the y axis, half and half between the identity and a 170 degree twist about y."""
    bind, lin, _ = _ring_case(frt, 170.0, "linear")
    r0 = np.hypot(bind[:, 0], bind[:, 2])
    rl = np.hypot(lin[:, 0], lin[:, 2])
    assert np.allclose(rl / r0, np.cos(np.radians(85.0)), atol=1e-6) and rl.max() < 0.09 * r0.max()      # the linear blend: 8.7 % of the radius is left
    bind, dq, (j, w, pal) = _ring_case(frt, 170.0, DQ)
    tol = BOUND * np.abs(bind[:, :3]).max()
    assert np.abs(np.hypot(dq[:, 0], dq[:, 2]) - r0).max() <= tol      # the distance from the axis
    assert np.abs(dq[:, 1] - bind[:, 1]).max() <= tol                  # the height
    want = bind[:, :3] @ rotation([0, 1, 0], np.radians(85.0)).T       # the ring turned by half the twist
    assert np.abs(dq - want).max() <= tol
    model, dec = skin_dq_model(bind, j, w, pal)
    assert np.abs(dq - model[:, :3]).max() <= tol and dec["sigma_margin"].min() > 0.08      # cos 85 degrees: 170, not 180, keeps sigma clear


def _posed(frt, pos, j, w, pal, mode=DQ):
    meshes = [mesh_of(frt, pos)]
    fs = scene_of(frt, meshes)
    fs.set_mesh_skin(0, j, w, num_joints=len(pal), mode=mode)
    fs.set_mesh_pose(0, pal)
    return posed_positions(fs, meshes, 0).astype(D)


def test_rigid_identities(frt):
    rng = np.random.default_rng(3)
    n = 33
    pos = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.ones((n, 1))], axis=1).astype(F)
    P = pos[:, :3].astype(D)
    # all four slots name one rigid joint: that joint's transform of the vertex
    R, t = rotation([1, 2, -0.5], 2.1), np.array([0.3, -0.2, 0.7])
    pal = np.stack([trs(), trs(R, t), trs()])
    j = np.full((n, 4), 1, np.uint16)
    w = random_weights(rng, n)
    w = (w / w.sum(axis=1, keepdims=True)).astype(F)
    got = _posed(frt, pos, j, w, pal)
    m = pal[1].astype(D).reshape(4, 4).T
    want = P @ m[:3, :3].T + m[:3, 3]
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    # 200 degrees and -160 degrees about one axis are one rotation: one pose (the quaternions are antipodal or equal; sigma sees to it)
    jj, ww = make_skin(n, 2)
    ax = [0.2, 1.0, 0.1]
    a = _posed(frt, pos, jj, ww, np.stack([trs(rotation(ax, 0.3)), trs(rotation(ax, np.radians(200.0)), t)]))
    b = _posed(frt, pos, jj, ww, np.stack([trs(rotation(ax, 0.3)), trs(rotation(ax, np.radians(-160.0)), t)]))
    assert np.abs(a - b).max() <= BOUND * np.abs(a).max()
    # S(0.01) R T against an inverse-bind-like S(100): the uniform scale is reproduced
    small = np.eye(4); small[:3, :3] = 0.01 * R; small[:3, 3] = 0.01 * (R @ t)
    palette = np.ascontiguousarray(small.T.reshape(1, 16), F)
    big = (100.0 * pos[:, :3]).astype(F)
    got = _posed(frt, np.concatenate([big, np.ones((n, 1), F)], axis=1), np.zeros((n, 4), np.uint16), w, palette)
    m = palette[0].astype(D).reshape(4, 4).T
    want = big.astype(D) @ m[:3, :3].T + m[:3, 3]
    assert np.abs(got - want).max() <= BOUND * np.abs(want).max()
    assert abs(joint_dq(palette[0])["s"] - 0.01) < 1e-8


def _family(name, rng, n):
    """(positions, joints, weights, palette) of one case family; the joints are drawn so that the model's sigma decisions are clear."""
    pos = np.concatenate([rng.uniform(-1, 1, (n, 3)), np.ones((n, 1))], axis=1).astype(F)
    w = random_weights(rng, n)
    if name == "rigid":
        pal = random_palette(rng, 24)
    elif name == "scaled":
        pal = random_palette(rng, 24, scale=(0.5, 2.0))
    elif name == "far":      # translations of 20: the dual part dominates
        pal = random_palette(rng, 24, scale=(0.5, 2.0), spread=20.0)
    else:
        pal = random_palette(rng, 24, scale=(0.5, 2.0))
    j = clear_skin(rng, n, pal, w, SIGMA_CLEAR)
    if name == "one joint":
        j[:] = j[:, :1]
    return pos, j, w, pal


def measure_f64(frt, seed=0, n=160):
    """{family: max|f32 - f64| / max|f64|}, and the smallest margins met; the cap on excluded vertices is zero: every vertex drawn is compared."""
    out, margins = {}, {"sigma": np.inf, "branch": np.inf, "branch_gap_when_near": 0.0}
    for k, name in enumerate(F64_MEASURED):
        rng = np.random.default_rng(100 * seed + k)
        pos, j, w, pal = _family(name, rng, n)
        got = _posed(frt, pos, j, w, pal)
        model, dec = skin_dq_model(pos, j, w, pal)
        assert got.shape == (n, 3) and np.isfinite(got).all()
        out[name] = float(np.abs(got - model[:, :3]).max() / np.abs(model[:, :3]).max())
        margins["sigma"] = min(margins["sigma"], float(dec["sigma_margin"].min()))
        for jd in dec["joints"]:
            margins["branch"] = min(margins["branch"], jd["branch_margin"])
            if jd["branch_margin"] < BRANCH_NEAR:
                margins["branch_gap_when_near"] = max(margins["branch_gap_when_near"], jd["runner_up_gap"])
        assert (w == 0).any() and (np.abs(w.sum(axis=1) - 1) > 0.1).any()
    return out, margins


def test_close_to_float64(frt):
    got, margins = measure_f64(frt)
    for name, err in got.items():
        print(f"{name}: {err:.3e} (measured {F64_MEASURED[name]:.3e})")
    assert margins["sigma"] >= SIGMA_CLEAR                              # every sigma decision of the data is clear, by the model alone
    assert margins["branch_gap_when_near"] <= BOUND                     # a Shepperd choice that is not clear is a choice between equals
    for name, err in got.items():
        assert err <= 4.0 * F64_MEASURED[name], (name, err)


def test_the_shepperd_branches_agree_where_they_meet():
    """Rotations built ON the boundaries between the branches (the angle about an axis at which t hands over to a diagonal entry, found by bisection), in float64: the two
    candidates give one quaternion within the bound, so whichever way f32 falls there, the pose is the same."""
    seen = set()
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.2], [0.3, 1, 1]):
        lo, hi = 0.1, np.pi - 1e-3      # the branch is t near 0 and a diagonal entry near pi (for these axes)
        b0 = joint_dq(trs(rotation(axis, lo)).astype(D))["branch"]
        assert b0 == 0 and joint_dq(trs(rotation(axis, hi)).astype(D))["branch"] != 0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if joint_dq(trs(rotation(axis, mid)).astype(D))["branch"] == 0:
                lo = mid
            else:
                hi = mid
        for ang in (lo, hi):
            jd = joint_dq(_mat64(rotation(axis, ang)))
            assert jd["branch_margin"] < 1e-9 and jd["runner_up_gap"] <= BOUND
            seen.add((jd["branch"], jd["runner_up"]))
    assert len(seen) >= 4


def _mat64(R):
    m = np.eye(4)
    m[:3, :3] = R
    return m.T.reshape(16)


def test_rejections_leave_the_scene_alone(frt):
    n = 12
    meshes = [ring_mesh(frt, n)]
    fs = scene_of(frt, meshes)
    j, w = make_skin(n, 3)
    j[j == 2] = 1                                   # no vertex names joint 2
    j[0, 0] = 0
    fs.set_mesh_skin(0, j, w, num_joints=3, mode=DQ)
    good = np.stack([trs(rotation([0, 1, 0], 0.4)), trs(rotation([1, 0, 0], -0.3), (0.1, 0.0, 0.0)), trs()])
    fs.set_mesh_pose(0, good)
    start = _state(fs)
    zero_col = good.copy(); zero_col[0, 4:7] = 0.0                      # a zero column in a joint vertices name
    with pytest.raises(frt.FrtError, match="not finite"):
        fs.set_mesh_pose(0, zero_col)
    unnamed = good.copy(); unnamed[2, 0:3] = 0.0                        # ... in a joint no vertex names: nothing reads it, the pose is the good one
    fs.set_mesh_pose(0, unnamed)
    assert _state(fs) == start
    with pytest.raises(frt.FrtError, match="not finite"):
        fs.set_mesh_pose(0, overflowing_palette(3))
    # a blend whose real part is exactly zero: every weight 0 (b_r = 0, rsqrt_exact(0) is an infinity, the coordinates NaN)
    wz = np.zeros((n, 4), F)
    fs2 = scene_of(frt, meshes)
    fs2.set_mesh_skin(0, j, wz, num_joints=3, mode=DQ)
    before = _state(fs2)
    with pytest.raises(frt.FrtError, match="not finite"):
        fs2.set_mesh_pose(0, good)
    # ... and weights so small that dot4(b_r, b_r) underflows to 0 although b_r is not 0
    fs2.set_mesh_skin(0, j, np.tile(F([1e-30, 1e-30, 0, 0]), (n, 1)), num_joints=3, mode=DQ)
    with pytest.raises(frt.FrtError, match="not finite"):
        fs2.set_mesh_pose(0, good)
    assert _state(fs2) == before and _state(fs) == start


def test_opposite_rotations_at_equal_weight_do_not_cancel(frt):
    """The contract's sigma makes a cancelling pair unreachable from matrices: with P the pivot, dot4(b_r, qr_P) = sum_k w_k |dot4(qr_k, qr_P)| >= w_P,
    and P has the greatest weight, so b_r is zero only when every weight is (the case above). Shown on the pairs that come nearest: turns of +a and -a
    about one axis at weights (0.5, 0.5) (a = 170 degrees: sigma flips one, the w components cancel exactly and a half turn is left; a = 60 degrees:
    the vector parts cancel and the identity is left), and turns of a and a + 180 degrees, whose quaternions are orthogonal. Each is posed, finite,
    and within the bound of the float64 model."""
    n = 12
    pos = ring_mesh(frt, n).positions
    j = np.tile(np.array([0, 1, 0, 0], np.uint16), (n, 1))
    w = np.tile(F([0.5, 0.5, 0.0, 0.0]), (n, 1))
    ax = [0.0, 1.0, 0.0]
    for a0, a1 in ((170.0, -170.0), (60.0, -60.0), (40.0, 220.0)):
        pal = np.stack([trs(rotation(ax, np.radians(a0))), trs(rotation(ax, np.radians(a1)))])
        got = _posed(frt, pos, j, w, pal)
        model, dec = skin_dq_model(pos, j, w, pal)
        assert np.isfinite(got).all() and np.abs(got - model[:, :3]).max() <= BOUND * np.abs(model[:, :3]).max(), (a0, a1)
    br = joint_dq(pal[0])["qr"] @ joint_dq(pal[1])["qr"]
    assert abs(br) < 1e-7      # (the last pair: orthogonal quaternions, the sigma decision is NOT clear, and either sign gives a finite pose)


def test_a_batch_mixes_the_modes_under_one_palette(frt):
    meshes = [ring_mesh(frt, 5), ring_mesh(frt, 70, 0.4), ring_mesh(frt, 9, 0.3)]
    skins = [make_skin(len(m.positions), 3, seed=k) for k, m in enumerate(meshes)]
    modes = ["linear", DQ, DQ]
    rng = np.random.default_rng(2)
    pal = random_palette(rng, 3, scale=(0.8, 1.2), spread=0.1, max_angle=1.0)
    a, b = scene_of(frt, meshes), scene_of(frt, meshes)
    for s in (a, b):
        for k in range(3):
            s.set_mesh_skin(k, *skins[k], num_joints=3, mode=modes[k])
    a.set_mesh_poses([2, 0, 1], pal)
    for k in (2, 0, 1):
        b.set_mesh_pose(k, pal)
    assert _state(a) == _state(b)
    lin = scene_of(frt, meshes)
    for k in range(3):
        lin.set_mesh_skin(k, *skins[k], num_joints=3)
    lin.set_mesh_poses([2, 0, 1], pal)
    assert _state(lin) != _state(a)
    assert posed_positions(lin, meshes, 0).tobytes() == posed_positions(a, meshes, 0).tobytes()      # the linear mesh of the mixed batch is the linear pose
    # morph, then skin, in either mode
    from _morph_model import make_targets, make_weights
    for s in (a, b):
        s.set_mesh_morph_targets(1, F(0.05) * make_targets(70, 2))
    a.set_mesh_poses([1], pal, make_weights(2))
    b.set_mesh_pose(1, pal, morph_weights=make_weights(2))
    assert _state(a) == _state(b)
    # the mode follows its mesh through remove_meshes (mesh 0 has an instance: take it away first)
    for s in (a, b):
        s.remove_instances([0])
        s.remove_meshes([0])
    a.set_mesh_poses([0, 1], pal)
    b.set_mesh_pose(0, pal); b.set_mesh_pose(1, pal)
    assert _state(a) == _state(b)
    got = a.get("tris")[:70, 0:3].astype(D)
    model, _ = skin_dq_model(meshes[1].positions, *skins[1], pal)
    assert np.abs(got - model[:, :3]).max() <= 4 * BOUND * np.abs(model[:, :3]).max()      # still the dual-quaternion pose, of the 70-vertex ring's own skin


def test_rigs_and_casts_pose_each_mesh_in_its_mode(frt):
    """scene.animate, animate_layers with a TwoBone goal and animate_cast over one linear and one dual-quaternion character are rig.evaluate*
    followed by the pose call, bit for bit."""
    from _blend_model import make_blend_rig
    from test_animation_ik import row
    meshes = [ring_mesh(frt, 40), ring_mesh(frt, 70, 0.4)]
    desc = make_blend_rig("tree12", nclips=3, seed=3, joints="subset", num_targets=0, keys=(2, 5), spread=0.2)
    desc["translations"] = F(0.1) * desc["translations"]
    rig = frt.Rig(**desc)
    a, b = scene_of(frt, meshes), scene_of(frt, meshes)
    for s in (a, b):
        for m, mode in ((0, "linear"), (1, DQ)):
            s.set_mesh_skin(m, *make_skin(len(meshes[m].positions), rig.num_joints, seed=m), num_joints=rig.num_joints, mode=mode)
    a.animate(rig, [0, 1], "c1", 0.45)
    b.set_mesh_poses([0, 1], *rig.evaluate("c1", 0.45))
    assert _state(a) == _state(b)
    par = np.asarray(desc["parents"])
    dep = np.zeros(len(par), int)
    for k, p in enumerate(par):
        dep[k] = 0 if p < 0 else dep[p] + 1
    tip = int(np.argmax(dep))
    goals = [frt.TwoBone(int(par[par[tip]]), int(par[tip]), tip)]
    t = np.stack([row(np.array([0.3, 0.2, 0.1]), 0.75)])
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    a.animate_layers(rig, [0, 1], layers, goals=goals, targets=t)
    b.set_mesh_poses([0, 1], *rig.evaluate_layers(layers, None, goals, t))
    assert _state(a) == _state(b)
    a.animate_cast([(rig, [0], "c2", 0.3), (rig, [1], "c0", 0.6)])
    b.set_mesh_poses([0], *rig.evaluate("c2", 0.3))
    b.set_mesh_poses([1], *rig.evaluate("c0", 0.6))
    assert _state(a) == _state(b)
    c = scene_of(frt, meshes)      # the same cast with both characters linear differs in the second mesh only
    for m in (0, 1):
        c.set_mesh_skin(m, *make_skin(len(meshes[m].positions), rig.num_joints, seed=m), num_joints=rig.num_joints)
    c.animate_cast([(rig, [0], "c2", 0.3), (rig, [1], "c0", 0.6)])
    assert posed_positions(c, meshes, 0).tobytes() == posed_positions(a, meshes, 0).tobytes()
    assert posed_positions(c, meshes, 1).tobytes() != posed_positions(a, meshes, 1).tobytes()


def test_bind_character_passes_the_mode_through(frt):
    class Model:
        def morph_targets(self, g):
            return None

        def skin(self, g):
            return make_skin(12, 3) + (0,)

        def skin_joints(self, s):
            return (list(range(3)),)

    class Target:
        calls = []

        def set_mesh_skin(self, *a, **kw):
            self.calls.append(kw)

    t = Target()
    assert frt.loader.bind_character(t, Model(), [4], skin_mode=DQ) == [4] and t.calls[-1]["mode"] == DQ
    assert frt.loader.bind_character(t, Model(), [4]) == [4] and t.calls[-1]["mode"] == "linear"


def test_host_form_runs_clean_under_a_sanitiser(tmp_path):
    """tools/skin_dq_sanitize.cpp with the host scene sources, stand-alone, with -fsanitize=address,undefined (the command line of ik_sanitize)."""
    csrc = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "csrc")
    exe = str(tmp_path / "skin_dq_sanitize")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math"] + san +
                   [os.path.join(ROOT, "tools", "skin_dq_sanitize.cpp"), os.path.join(csrc, "frt_scene.cpp"), os.path.join(csrc, "frt_bvh.cpp"),
                    "-fsanitize=address,undefined", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok: "), run.stdout + run.stderr
