"""The animation on the device (include/frt.h: frt_renderer_bind_rig, frt_renderer_animate; DESIGN.md section 11, "Animation"): the kernel's palette and
weights are frt_rig_evaluate's, bit for bit, on the rig shapes at which it could go wrong; after animate the replica equals the host scene after
SceneBuilder.animate and a renderer fed the host-evaluated values as device tensors; a frame equals that of a renderer created from the posed host
scene; an overflowing clip is rejected on the device and counted; what cannot be animated is refused on the host; a MultiRenderer's strips follow.
Tiny frames on the scene with a spare mesh."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_skin_gpu import torch_dev, check_replica, _replica, _up, EVERY, W, H      # noqa: F401  (torch_dev: a fixture)
from _skin_model import F, make_skin, scene_with_a_spare_mesh
from _morph_model import make_targets
from _anim_model import make_rig, make_channel, sample_times

pytestmark = pytest.mark.gpu
SPARE = 1            # the crystal: in the pools, no instance
CHARACTER = [2, 3]   # the two spheres, 162 and 42 vertices, one instance each (one mirrored)

# (shape, joints, targets): the smallest rigs at which the kernel can go wrong
SHAPES = {"one node": ("chain1", "all", 3), "more levels than a wave has lanes": ("chain70", "all", 3), "a level past the wave": ("fan65", "all", 3),
          "past the workgroup": ("tree257", "all", 3), "the LDS limit": ("tree1024", "all", 3), "joints a permuted strict subset": ("tree257", "subset", 3),
          "morph only": ("chain2", "none", 5), "skin only": ("tree257", "all", 0)}


def bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32).tolist()


def bind_synthetic(frt, target, meshes, ids, rig, seed=0):
    """For the synthetic rigs no file holds (frt.loader.bind_character binds a loaded document's own arrays): what the rig implies, bound to every mesh of `ids`: a skin of rig.num_joints joints and / or rig.num_targets small targets."""
    for m in ids:
        n = len(meshes[m].positions)
        if rig.num_targets:
            target.set_mesh_morph_targets(m, F(0.05) * make_targets(n, rig.num_targets, seed=seed + m))
        if rig.num_joints:
            target.set_mesh_skin(m, *make_skin(n, rig.num_joints, seed=seed + m), num_joints=rig.num_joints)


def character_rig(frt, extra_channels=(), seed=3):
    """A 12-node rig near the identity (the posed spheres stay about where they were), all three interpolations, 3 targets."""
    desc = make_rig("tree12", seed=seed, joints="subset", num_targets=3, keys=(2, 5))
    desc["translations"] = F(0.1) * desc["translations"]
    desc["rotations"] = np.tile(F([0, 0, 0, 1]), (12, 1)) + F(0.05) * desc["rotations"]
    for ch in desc["clips"][0][1]:
        if ch["path"] == "translation":
            ch["values"] = F(0.2) * ch["values"]
        if ch["path"] == "rotation":
            ch["values"] = F([0, 0, 0, 1]) + F(0.1) * ch["values"]
            ch["values"] = (ch["values"] / np.linalg.norm(ch["values"], axis=-1, keepdims=True)).astype(F)
            if ch["interpolation"] == "CUBICSPLINE":
                ch["values"][:, 0::2] = F(0.02) * ch["values"][:, 0::2]
    desc["clips"] = desc["clips"] + list(extra_channels)
    return desc


@pytest.mark.parametrize("which", list(SHAPES))
def test_palette_and_weights_have_the_host_bits(gpu, which):
    frt = gpu
    shape, joints, targets = SHAPES[which]
    desc = make_rig(shape, joints=joints, num_targets=targets, keys=(1, 2, 33))
    rig = frt.Rig(**desc)
    assert {c["interpolation"] for c in desc["clips"][0][1]} == {"STEP", "LINEAR", "CUBICSPLINE"} or shape == "chain2"
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    bind_synthetic(frt, r, meshes, [SPARE], rig)
    b = r.bind_rig(rig, [SPARE])
    for clip, times in ((0, sample_times(desc, 10)), (1, F([0.0]))):      # before, after, at and between the keys; then the clip without channels
        for t in times:
            r.animate(b, clip, t)
            got, want = r.read_rig_pose(b), rig.evaluate(clip, t)
            assert bits(got[0]) == bits(want[0]), f"{which}: palette, clip {clip} at {t}"
            assert bits(got[1]) == bits(want[1]), f"{which}: weights, clip {clip} at {t}"
    assert r.deform_rejects() == 0
    r.unbind_rig(b)
    with pytest.raises(frt.FrtError):
        r.animate(b, 0, 0.0)


def loaded_character(frt, tmp_path):
    """(host scene, model, mesh ids): the two-primitive character of tests/_gltf_rig.py, loaded, as two meshes with one instance each (one mirrored)
    beside a floor and a light."""
    from _gltf_rig import character
    from frt.scenes import _T, _S, _RX, _mul
    w, _ = character()
    path = tmp_path / "character.glb"
    w.save_glb(str(path))
    model = frt.loader.load_gltf(path)
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.create_plane())
    ids = [b.add_mesh(model.geometry(g)[0]) for g in range(2)]
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(0, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.register_quad_light(0, _mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.5)), (1.0, 1.0, 1.0), 10.0)
    b.add_instance(ids[0], grey, _mul(_T(-0.4, -0.3, 0.0), _S(1.5)))
    b.add_instance(ids[1], grey, _mul(_T(0.4, -0.3, 0.1), np.diag(np.array([-1.5, 1.5, 1.5, 1.0], F))))
    return b.build(), model, ids


def test_replica_equals_the_host_scene_and_the_tensor_route(gpu, torch_dev, tmp_path):
    """A loaded document end to end: load_gltf, bind_character, Model.rig, bind_rig, animate."""
    frt = gpu
    torch, dev = torch_dev
    fs, model, ids = loaded_character(frt, tmp_path)
    rig = model.rig(0)
    assert (rig.num_joints, rig.num_targets) == (5, 2)
    r, other = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render(cam)
    start = r.read_scene("tri_slots").tobytes()
    for x in (r, other, fs):
        assert frt.loader.bind_character(x, model, ids) == ids
    b = r.bind_rig(rig, ids)
    for clip, t in (("wave", -1.0), ("wave", 0.5), ("nod", 0.8)):      # before the keys, at a key, between keys
        r.animate(b, clip, t)
        fs.animate(rig, ids, clip, t)
        pal, w = rig.evaluate(clip, t)
        got = r.read_rig_pose(b)
        assert bits(got[0]) == bits(pal) and bits(got[1]) == bits(w)
        other.set_mesh_poses(ids, _up(torch, dev, pal), _up(torch, dev, w))      # the only other route to the same replica
        check_replica(frt, r, fs, f"animate {clip} at {t}")
        got, want = _replica(r), _replica(other)
        for x in EVERY:
            assert got[x] == want[x], f"animate vs set_mesh_poses with tensors, {clip} at {t}: {x}"
    assert r.read_scene("tri_slots").tobytes() != start and r.deform_rejects() == 0
    r.clear()
    rf = frt.Renderer(fs, W, H, max_depth=8, flags=frt.FLAG_PIPELINE)      # from the posed host scene
    r.render(cam); rf.render(cam)
    compare_all(r.read_buffer, rf.read_buffer, 0, "an animated replica vs a renderer created from the posed host scene")


def test_a_binding_follows_remove_meshes_and_numbers_are_reused(gpu):
    frt = gpu
    desc = character_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r, ref = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    for x in (r, ref):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
        bind_synthetic(frt, x, meshes, [SPARE], rig)
    b, lost = r.bind_rig(rig, CHARACTER), r.bind_rig(rig, [SPARE])
    assert (b, lost) == (0, 1)
    for x in (r, ref):
        x.remove_meshes([SPARE])                       # 2 and 3 become 1 and 2; the binding of the mesh that left is unbound
    assert frt.lib().frt_renderer_animate(r._h, lost, 0, 0.5, 0) == -1
    r.animate(b, "move", 0.5)
    ref.set_mesh_poses([1, 2], *rig.evaluate("move", 0.5))
    got, want = _replica(r), _replica(ref)
    for x in EVERY:
        assert got[x] == want[x], x
    assert r.bind_rig(rig, [1, 2]) == 1               # the freed number is used again
    r.unbind_rig(0)
    assert r.bind_rig(rig, [1]) == 0 and r.deform_rejects() == 0


def test_an_overflowing_clip_is_rejected_on_the_device(gpu):
    frt = gpu
    desc = character_rig(frt)
    big = {"node": 0, "path": "scale", "interpolation": "LINEAR", "times": F([0.0, 1.0]), "values": F([[1, 1, 1], [3e38, 3e38, 3e38]])}
    desc["scales"][1:] = 4.0      # under the root's 3e38 every other node's global overflows
    desc["clips"].append(("burst", [big]))
    rig = frt.Rig(**desc)
    assert not np.isfinite(rig.evaluate("burst", 1.0)[0]).all() and np.isfinite(rig.evaluate("burst", 0.0)[0]).all()
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for x in (r, fs):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b = r.bind_rig(rig, CHARACTER)
    r.animate(b, "burst", 0.0); fs.animate(rig, CHARACTER, "burst", 0.0)
    start = _replica(r)
    r.animate(b, "burst", 1.0)
    assert r.deform_rejects() == 1
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], f"a rejected animate changed {x}"
    with pytest.raises(frt.FrtError):
        fs.animate(rig, CHARACTER, "burst", 1.0)
    r.animate(b, "move", 0.4); fs.animate(rig, CHARACTER, "move", 0.4)      # and a valid one applies
    assert r.deform_rejects() == 1 and r.read_scene("tri_slots").tobytes() != start["tri_slots"]
    check_replica(frt, r, fs, "a valid animate after a rejected one")


def test_refusals(gpu):
    frt = gpu
    L = frt.lib()
    desc = character_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    r = frt.Renderer(fs, W, H)
    start = _replica(r)
    with pytest.raises(frt.FrtError, match="error -1"):      # no mesh has what the rig implies
        r.bind_rig(rig, CHARACTER)
    bind_synthetic(frt, r, meshes, CHARACTER[:1], rig)
    with pytest.raises(frt.FrtError, match="error -1"):      # the last mesh of the list has not
        r.bind_rig(rig, CHARACTER)
    bind_synthetic(frt, r, meshes, CHARACTER[1:], rig)
    other = frt.Rig(**make_rig("chain2", num_targets=3))      # another joint count
    too_many = frt.Rig(**make_rig("chain1025", num_targets=0))
    assert too_many.num_nodes == frt.MAX_RIG_NODES + 1
    for bad, ids in ((other, CHARACTER), (too_many, CHARACTER), (rig, []), (rig, [2, 2]), (rig, [2, 99])):
        with pytest.raises(frt.FrtError, match="error -1"):
            r.bind_rig(bad, ids)
    b = r.bind_rig(rig, CHARACTER)
    call = L.frt_renderer_animate
    assert call(r._h, b + 1, 0, 0.0, 0) == -1                               # an unknown binding
    assert call(r._h, b, rig.num_clips, 0.0, 0) == -1                       # clip out of range
    for t in (np.nan, np.inf, -np.inf):
        assert call(r._h, b, 0, t, 0) == -1                                 # a time that is not finite
    assert call(r._h, b, 0, 0.0, frt.DEFORM_DEVICE) == -1 and call(r._h, b, 0, 0.0, 4) == -1      # flags animate does not take
    assert call(None, b, 0, 0.0, 0) == -1
    r.set_mesh_skin(CHARACTER[1], None)                                     # a mesh of the list loses its skin
    assert call(r._h, b, 0, 0.0, 0) == -1
    r.set_mesh_skin(CHARACTER[1], *make_skin(len(meshes[CHARACTER[1]].positions), rig.num_joints + 1), num_joints=rig.num_joints + 1)
    assert call(r._h, b, 0, 0.0, 0) == -1                                   # ... or has another joint count
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    bind_synthetic(frt, r, meshes, CHARACTER[1:], rig)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    assert call(r._h, b, 0, 0.0, 0) == -4                                   # inside an open frame
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert r.deform_rejects() == 0
    now = _replica(r)
    for x in EVERY:
        assert now[x] == start[x], x
    r.animate(b, "move", 0.5, normals="keep")                               # and the good call applies
    assert r.deform_rejects() == 0 and r.read_scene("tri_slots").tobytes() != start["tri_slots"]


def test_multi_renderer(gpu):
    """Two strips on one device: every strip's rows of the frame equal those of a single renderer animated on the device."""
    frt = gpu
    desc = character_rig(frt)
    rig = frt.Rig(**desc)
    fs, meshes, _ = scene_with_a_spare_mesh(frt)
    multi, one = frt.MultiRenderer(fs, 64, 48, [0, 0]), frt.Renderer(fs, 64, 48, flags=frt.FLAG_PIPELINE)
    for x in (multi, one):
        bind_synthetic(frt, x, meshes, CHARACTER, rig)
    b = one.bind_rig(rig, CHARACTER)
    for t in (0.3, 0.6):
        multi.animate(rig, CHARACTER, "move", t)
        one.animate(b, "move", t)
        for x in (multi, one):
            x.clear()
            x.render(frt.CameraController().build_uniform(64 / 48, 0, fs.num_lights))
        multi.sync()
        assert multi.read_accum().tobytes() == one.read_accum().tobytes(), t
