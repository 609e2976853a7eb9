"""Dual-quaternion skinning on the device (include/frt.h: frt_renderer_set_mesh_skin_ex, FRT_SKIN_DUAL_QUATERNION; DESIGN.md section 11,
"Dual-quaternion skinning"): after the same binds and the same calls the replica equals the host scene bit for bit, for every route that ends in a
pose, on meshes of 5, 70 and 257 vertices added to the Cornell Box so that one wave of the pose kernels holds vertices of a linear and of a
dual-quaternion segment, a segment crosses a wave and a block boundary and the last block is ragged; what the host refuses the device rejects, counted
once and with nothing applied, whichever skin kernel runs first; the mode follows its mesh through remove_meshes; frames equal those of a scene built
from scratch with the host-posed vertices. Tiny frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import cornell_with, SPHERE, QUAD_LIGHT, SPHERE_LIGHT
from test_mesh_normals_gpu import check_replica, W, H
from _skin_model import F, make_skin
from _morph_model import make_targets, make_weights
from _blend_model import make_blend_rig, random_blends
from _skin_dq_model import random_palette, ring_mesh, trs, rotation

pytestmark = pytest.mark.gpu
DQ = "dual_quaternion"
A, B, C = 4, 5, 6                                   # the added meshes: 5, 70 and 257 vertices
SIZES = {A: 5, B: 70, C: 257}
MODES = {A: "linear", B: DQ, C: DQ}                 # a batch [A, B, C]: vertices 0 .. 4 linear and 5 .. 63 dual-quaternion in wave 0; B ends in wave 1;
NJ = 6                                              # C runs from 75 to 331, across the block boundary at 256; 332 vertices: a ragged second block


def _rings(frt):
    return [ring_mesh(frt, 5, 0.2, 0.1), ring_mesh(frt, 70, 0.3, 0.15), ring_mesh(frt, 257, 0.4, 0.2, turns=3)]


def _skins(nj=NJ):
    return {m: make_skin(n, nj, seed=m) for m, n in SIZES.items()}


def _host_scene(frt, extra):
    """cornell_with, with `extra` meshes appended and one identity instance of each (material 0) behind the box's own: world triangles of the added
    meshes are their object-space positions."""
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    b = frt.SceneBuilder()
    for g in cornell_meshes(frt) + list(extra):
        b.add_mesh(g)
    for k in range(6):
        b.add_material(frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()))
    for k, row in enumerate(inst):
        m = row[5:21].view(np.float32)
        if k == QUAD_LIGHT:
            b.register_quad_light(int(row[0]), m, (1.0, 1.0, 1.0), 10.0)
        elif k == SPHERE_LIGHT:
            b.register_sphere_light(int(row[0]), m, (0.02, 0.02, 0.9), 10.0)
        else:
            b.add_instance(int(row[0]), int(row[1]), m)
    for k in range(len(extra)):
        b.add_instance(4 + k, 0, np.eye(4, dtype=F).reshape(16))
    return b.build()


def _world(frt, modes=MODES, nj=NJ, morph=()):
    """(renderer, host scene): the Cornell Box, the three rings added between frames, skins bound in `modes`, targets on the meshes of `morph`."""
    rings = _rings(frt)
    assert len(cornell_meshes(frt)) == 4
    fs = _host_scene(frt, rings)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=2)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    assert r.add_meshes(rings) == A
    r.add_instances([A, B, C], [0, 0, 0], np.tile(np.eye(4, dtype=F).reshape(16), (3, 1)))
    skins = _skins(nj)
    for x in (r, fs):
        for m, mode in modes.items():
            x.set_mesh_skin(m, *skins[m], num_joints=nj, mode=mode)
        for m in morph:
            x.set_mesh_morph_targets(m, F(0.02) * make_targets(SIZES[m], 2, seed=m))
    return r, fs


def _pal(seed, nj=NJ):
    return random_palette(np.random.default_rng(seed), nj, scale=(0.8, 1.25), spread=0.1, max_angle=2.5)


def _both(r, fs, call, *args, **kw):
    getattr(r, call)(*args, **kw); getattr(fs, call)(*args, **kw)


def _up(torch, r, a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(f"cuda:{r.device}")


def test_poses_and_batches(gpu):
    frt = gpu
    import torch
    r, fs = _world(frt, morph=(B,))
    for m in (A, B, C):                                     # single calls from host matrices: a linear mesh, then the two dual-quaternion ones
        _both(r, fs, "set_mesh_pose", m, _pal(m))
    check_replica(frt, r, fs, "set_mesh_pose from host matrices", rebuilt=True)
    for m in (B, C, A):                                     # ... and from a device tensor
        pal = _pal(10 + m)
        r.set_mesh_pose(m, _up(torch, r, pal), normals="keep"); fs.set_mesh_pose(m, pal, normals="keep")
    check_replica(frt, r, fs, "set_mesh_pose from a device tensor", rebuilt=True)
    _both(r, fs, "set_mesh_poses", [A, B, C], _pal(20))      # mixed modes under one palette: both skin kernels run, the linear one first
    check_replica(frt, r, fs, "a mixed batch", rebuilt=True)
    pal = _pal(21)
    r.set_mesh_poses([C, A, B], _up(torch, r, pal)); fs.set_mesh_poses([C, A, B], pal)
    check_replica(frt, r, fs, "a mixed batch from a device tensor", rebuilt=True)
    _both(r, fs, "set_mesh_poses", [B, C], _pal(22))         # dual-quaternion only: the linear kernel does not run
    check_replica(frt, r, fs, "a dual-quaternion batch", rebuilt=True)
    _both(r, fs, "set_mesh_pose", B, _pal(23), morph_weights=make_weights(2))      # morph, then dual-quaternion skin
    check_replica(frt, r, fs, "morph then skin", rebuilt=True)
    pal = _pal(24)
    _both(r, fs, "set_mesh_poses", [A, B], pal)              # 75 vertices: one wave with both modes and a ragged second one
    check_replica(frt, r, fs, "a wave with both modes", rebuilt=True)
    assert r.deform_rejects() == 0


def test_rigs_and_casts(gpu):
    frt = gpu
    desc = make_blend_rig("tree12", nclips=3, seed=3, joints="subset", num_targets=0, keys=(2, 5), spread=0.2)
    desc["translations"] = F(0.1) * desc["translations"]
    rig = frt.Rig(**desc)
    r, fs = _world(frt, nj=rig.num_joints)
    both, lin, dq = r.bind_rig(rig, [A, B, C]), None, None
    r.animate(both, "c1", 0.45); fs.animate(rig, [A, B, C], "c1", 0.45)
    check_replica(frt, r, fs, "animate", rebuilt=True)
    blend = random_blends(desc, 3, 1, seed=2)[0]
    r.animate_blend(both, blend); fs.animate_blend(rig, [A, B, C], blend)
    check_replica(frt, r, fs, "animate_blend", rebuilt=True)
    par = np.asarray(desc["parents"])
    dep = np.zeros(len(par), int)
    for k, p in enumerate(par):
        dep[k] = 0 if p < 0 else dep[p] + 1
    tip = int(np.argmax(dep))
    goals = [frt.TwoBone(int(par[par[tip]]), int(par[tip]), tip)]
    rows = np.zeros((1, 8), F)
    rows[0, :4] = (0.3, 0.2, 0.1, 0.75)
    layers = [("c0", 0.4, 1.0), frt.Layer("c1", 0.5, 0.5, mode="override")]
    r.set_rig_goals(both, goals); r.set_rig_goal_targets(both, rows)
    r.animate_layers(both, layers); fs.animate_layers(rig, [A, B, C], layers, goals=goals, targets=rows)
    check_replica(frt, r, fs, "animate_layers with a goal", rebuilt=True)
    r.unbind_rig(both)
    lin, dq = r.bind_rig(rig, [A]), r.bind_rig(rig, [B, C])      # a cast with one character of each mode
    r.animate_cast([(lin, "c2", 0.3), (dq, "c0", 0.6)]); fs.animate_cast([(rig, [A], "c2", 0.3), (rig, [B, C], "c0", 0.6)])
    check_replica(frt, r, fs, "animate_cast", rebuilt=True)
    assert r.deform_rejects() == 0


def _scene(r):
    return {w: r.read_scene(w).tobytes() for w in ("tri_slots", "quad_nodes", "shade_tris", "attributes", "normals")}


def test_rejections_on_the_device(gpu):
    frt = gpu
    import torch
    r, fs = _world(frt, modes={B: DQ, C: DQ})
    skins = _skins()
    jb, wb = skins[B]
    jb = jb.copy(); jb[jb == 3] = 2                          # no vertex of B names joint 3
    jc = skins[C][0].copy(); jc[jc == 3] = 2
    for x in (r, fs):
        x.set_mesh_skin(B, jb, wb, num_joints=NJ, mode=DQ)
        x.set_mesh_skin(C, jc, skins[C][1], num_joints=NJ, mode=DQ)
    _both(r, fs, "set_mesh_poses", [B, C], _pal(1))
    start = _scene(r)
    good = _pal(2)
    nan_unnamed = good.copy(); nan_unnamed[3, 5] = np.nan    # a dual-quaternion-only batch: the palette test must have moved to its kernel
    r.set_mesh_poses([B, C], _up(torch, r, nan_unnamed))
    assert r.deform_rejects() == 1 and _scene(r) == start
    r.set_mesh_pose(B, _up(torch, r, nan_unnamed))
    assert r.deform_rejects() == 2 and _scene(r) == start
    zero_col = good.copy(); zero_col[2, 4:7] = 0.0           # a zero column in a joint vertices name: finite input, NaN coordinates
    assert (jb == 2).any()
    with pytest.raises(frt.FrtError, match="error -1"):
        fs.set_mesh_pose(B, zero_col)
    r.set_mesh_pose(B, _up(torch, r, zero_col))
    assert r.deform_rejects() == 3 and _scene(r) == start
    r.set_mesh_pose(B, zero_col)                             # ... from host memory too: the matrices are finite, the device finds the pose is not
    assert r.deform_rejects() == 4 and _scene(r) == start
    zero_unnamed = good.copy(); zero_unnamed[3, 0:3] = 0.0   # ... in a joint no vertex names: nothing reads it
    r.set_mesh_poses([B, C], _up(torch, r, zero_unnamed)); fs.set_mesh_poses([B, C], zero_unnamed)
    assert r.deform_rejects() == 4
    check_replica(frt, r, fs, "the next valid pose", rebuilt=True)
    # a mixed batch with the NaN: the linear kernel runs first and tests the palette, once
    for x in (r, fs):
        x.set_mesh_skin(A, *skins[A], num_joints=NJ)
    now = _scene(r)
    r.set_mesh_poses([A, B, C], _up(torch, r, nan_unnamed))
    assert r.deform_rejects() == 5 and _scene(r) == now
    _both(r, fs, "set_mesh_poses", [A, B, C], good)
    check_replica(frt, r, fs, "a valid mixed batch after a rejected one", rebuilt=True)
    for flags in (2, 5):                                     # refused on the host: an unknown flag bit
        assert frt.lib().frt_renderer_set_mesh_skin_ex(r._h, B, jb.ctypes.data, wb.ctypes.data, 70, NJ, flags) == -1
    with pytest.raises(frt.FrtError, match="mode must be"):
        r.set_mesh_skin(B, jb, wb, num_joints=NJ, mode="quaternion")
    assert r.deform_rejects() == 5


def test_the_mode_follows_its_mesh(gpu):
    """A, the linear mesh and the lowest id of the three, loses its instance and is removed: B and C (dual-quaternion) become 4 and 5 and must still
    pose in their mode, each with its own skin."""
    frt = gpu
    r, _ = _world(frt)
    n_inst = r.scene_counts()["instances"]
    r.remove_instances([n_inst - 3])
    r.remove_meshes([A])
    rings = _rings(frt)
    fs = _host_scene(frt, rings[1:])
    skins = _skins()
    fs.set_mesh_skin(4, *skins[B], num_joints=NJ, mode=DQ)
    fs.set_mesh_skin(5, *skins[C], num_joints=NJ, mode=DQ)
    _both(r, fs, "set_mesh_poses", [4, 5], _pal(3))
    check_replica(frt, r, fs, "after remove_meshes", rebuilt=True)
    lin = _host_scene(frt, rings[1:])                        # the same with linear skins differs: the mode did follow
    lin.set_mesh_skin(4, *skins[B], num_joints=NJ)
    lin.set_mesh_skin(5, *skins[C], num_joints=NJ)
    lin.set_mesh_poses([4, 5], _pal(3))
    assert lin.get("tris").tobytes() != fs.get("tris").tobytes()
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_pose(6, _pal(3))


def test_frames_equal_a_scene_built_from_scratch(gpu):
    frt = gpu
    base = cornell_meshes(frt)
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
    n = len(base[SPHERE].positions)
    skin = make_skin(n, 2)
    pal = np.stack([trs(), trs(rotation([0, 1, 0], np.radians(120.0)), (0.05, 0.0, 0.0))])      # a twist the linear blend would flatten
    _both(r, fs, "set_mesh_skin", SPHERE, *skin, num_joints=2, mode=DQ)
    _both(r, fs, "set_mesh_pose", SPHERE, pal)
    # the host-posed vertices: an identity-placed copy of the sphere in a scene of its own gives them back as its triangles' first vertices
    from _skin_dq_model import mesh_of, scene_of, posed_positions
    probe_mesh = [mesh_of(frt, base[SPHERE].positions)]
    probe = scene_of(frt, probe_mesh)
    probe.set_mesh_skin(0, *skin, num_joints=2, mode=DQ)
    probe.set_mesh_pose(0, pal)
    p = np.concatenate([posed_positions(probe, probe_mesh, 0), base[SPHERE].positions[:, 3:4]], axis=1).astype(F)
    mi = fs.get("mesh_infos")[SPHERE]
    meshes = list(base)
    meshes[SPHERE] = frt.geometry.Geometry(p, fs.get("attributes")[mi[0]:mi[0] + n].copy(), base[SPHERE].indices)
    fresh = cornell_with(frt, meshes)
    assert fresh.get("shade_tris").tobytes() == fs.get("shade_tris").tobytes() and fresh.get("tris").tobytes() == fs.get("tris").tobytes()
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "a dual-quaternion pose vs a build from scratch")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"])
