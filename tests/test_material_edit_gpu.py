"""Editing what a renderer's scene replica looks like (include/frt.h: frt_renderer_set_materials, _set_instance_materials, _set_light_emission,
_set_texture): the edited replica equals the host scene after the same edit byte for byte, an edited renderer renders exactly
what a fresh renderer over a scene built from scratch renders (and what the brute-force oracle renders), the two-stream schedule drops the frame that
ran ahead under the old values, and the queries see a new instance material at once.

The frame tests give the CRYSTAL another material: the Cornell Box's only sphere is the registered sphere light, which set_instance_materials refuses."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes, cornell_moves, QUAD_LIGHT, CRYSTAL, SPHERE_LIGHT, TALL_BOX
from test_material_edit import (cornell_look, cornell_edit, apply_edit, material, checker_texture, gradient_texture, RED, GREEN, WHITE, CHECKER, METAL,
                                GLASS, QUAD_LIGHT_MAT, FLOOR)

pytestmark = pytest.mark.gpu
LOOK = ("materials", "lights", "instances_dev", "shade_tris")
TREE = ("tri_slots", "quad_nodes")


@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


def assert_replica(r, fs, tree, ctx):
    for w in LOOK:
        got, want = r.read_scene(w), fs.get(w)
        assert got.tobytes() == want.tobytes(), f"{ctx}: {w}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
    for w in TREE:
        assert r.read_scene(w).tobytes() == tree[w], f"{ctx}: {w} changed"


def both(r, fs, method, *args):
    getattr(r, method)(*args)
    getattr(fs, method)(*args)


def test_replica_after_each_edit_on_the_cornell_box(gpu):
    frt = gpu
    fs = cornell_look(frt, color_textures=[gradient_texture()])
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    tree = {w: r.read_scene(w).tobytes() for w in TREE}
    assert_replica(r, fs, tree, "at create")
    cam = frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights)
    r.render(cam)                                                        # (the next frame's G-buffer + T-trace now run ahead)
    blue, rough, last = material(frt, [0.1, 0.2, 0.9, 1.0]), material(frt, [0.7, 0.7, 0.7, 1.0], roughness=0.9, texture=3), material(frt, [0.9, 0.6, 0.2, 1.0], metallic=1.0)
    both(r, fs, "set_materials", [METAL, RED, METAL, GREEN, QUAD_LIGHT_MAT - 1], [blue, rough, last, blue, rough])   # runs 0-1, 4-5; METAL twice
    assert_replica(r, fs, tree, "set_materials")
    assert r.read_scene("materials")[METAL].tobytes() == bytes(last)
    both(r, fs, "set_materials", list(range(6)), [rough, blue, last, rough, blue, last])                # one run
    assert_replica(r, fs, tree, "set_materials, all")
    both(r, fs, "set_instance_materials", [TALL_BOX, CRYSTAL, TALL_BOX], [RED, GREEN, CHECKER])           # 12 + 16 triangles, TALL_BOX twice
    assert_replica(r, fs, tree, "set_instance_materials")
    assert r.read_scene("instances_dev")[TALL_BOX, 1] == CHECKER
    r.render(cam)
    both(r, fs, "set_instance_materials", [FLOOR], [WHITE])                                               # the smallest instance alone: 2 triangles
    assert_replica(r, fs, tree, "set_instance_materials, floor")
    both(r, fs, "set_light_emission", 0, (1.0, 0.9, 0.8), 5.0)
    both(r, fs, "set_light_emission", 1, (0.9, 0.1, 0.3), 2.5)
    assert_replica(r, fs, tree, "set_light_emission")
    both(r, fs, "set_texture", "color", 3, checker_texture(64))
    both(r, fs, "set_texture", "data", 2, gradient_texture())
    assert_replica(r, fs, tree, "set_texture")
    r.set_materials([], []); r.set_instance_materials([], [])
    assert_replica(r, fs, tree, "empty calls")
    r.rebuild_tree(quality="sah")
    tree = {w: r.read_scene(w).tobytes() for w in TREE}
    both(r, fs, "set_instance_materials", [CRYSTAL, TALL_BOX, 1], [GLASS, METAL, RED])
    both(r, fs, "set_materials", [GLASS], [blue])
    assert_replica(r, fs, tree, "after rebuild_tree")


def test_replica_after_set_instance_materials_on_the_82k_blob(gpu, orc):
    """Instances: five walls and the light quad of 2 triangles each, the blob of 81,920. [wall, blob] is the smallest and the largest instance, 81,922
    triangles: 320 full blocks of 256 and a tail of 2; [blob, wall, wall] puts the binary search's boundary inside the last block."""
    frt = gpu
    import _scenes
    fs, _ = _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    tree = {w: r.read_scene(w).tobytes() for w in TREE}
    cam = frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights)
    r.render(cam)
    BLOB = 6
    assert fs.get("instances")[BLOB, 3] == 81920 and fs.get("instances")[0, 3] == 2
    both(r, fs, "set_instance_materials", [0, BLOB], [1, 2])
    assert_replica(r, fs, tree, "wall + blob")
    assert (r.read_scene("shade_tris")[fs.get("instances")[BLOB, 2]:, 25].view(np.uint32) == 2).all()
    both(r, fs, "set_instance_materials", [BLOB, 3, 1, BLOB], [0, 0, 2, 1])
    assert_replica(r, fs, tree, "blob + two walls, blob twice")
    both(r, fs, "set_instance_materials", [4], [0])
    assert_replica(r, fs, tree, "one wall")
    r.rebuild_tree(quality="sah")
    tree = {w: r.read_scene(w).tobytes() for w in TREE}
    both(r, fs, "set_instance_materials", [2, BLOB, 0], [1, 0, 0])
    assert_replica(r, fs, tree, "after rebuild_tree")


def oracle_scene(orc, fs, meshes, color_textures):
    """The oracle's own scene from the product scene's materials, lights and instances and the same extra colour layers (nothing of its tree)."""
    from _oracle import OrcScene
    oh = orc.L.orc_scene_create()
    for t in color_textures:
        t = np.ascontiguousarray(t, np.uint8); orc.L.orc_scene_add_texture(oh, 0, t.ctypes.data)
    for g in meshes:
        pos = np.ascontiguousarray(g.positions, np.float32); att = np.ascontiguousarray(g.attributes, np.float32); idx = np.ascontiguousarray(g.indices, np.uint32)
        orc.L.orc_scene_add_mesh(oh, pos.ctypes.data, pos.shape[0], att.ctypes.data, idx.ctypes.data, idx.size)
    for row in fs.get("materials"):
        m = np.ascontiguousarray(row); orc.L.orc_scene_add_material(oh, m.ctypes.data)
    for row in fs.get("lights"):
        l = np.ascontiguousarray(row); orc.L.orc_scene_add_light(oh, l.ctypes.data)
    for row in fs.get("instances"):
        m = np.ascontiguousarray(row[5:21]); orc.L.orc_scene_add_instance(oh, int(row[0]), int(row[1]), m.ctypes.data)
    orc.L.orc_scene_build(oh)
    return OrcScene(orc, oh)


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_edited_renderer_matches_a_fresh_build_and_the_oracle(gpu, orc, flags):
    frt = gpu
    W, H, depth, frames = 96, 64, 8, 3
    edit = cornell_edit(frt)
    fresh = cornell_look(frt, edit[0], edit[1], edit[2], color_textures=[edit[3]])
    r = frt.Renderer(cornell_look(frt, color_textures=[gradient_texture()]), W, H, max_depth=depth, flags=flags)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, fresh.num_lights))
    apply_edit(r, edit)
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=flags)
    ro = oracle_scene(orc, fresh, cornell_meshes(frt), [edit[3]]).renderer(W, H, depth, False, 16)      # brute force: nothing of any tree
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam); ro.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "edited vs fresh build")
        compare_all(r.read_buffer, ro.read, f, "edited vs brute-force oracle")
    st, sf, so = r.stats(), rf.stats(), ro.stats()["total"]
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"]) == (so["closest"], so["any"])
    # and the edit shows: a renderer over the unedited scene renders another image
    r0 = frt.Renderer(cornell_look(frt, color_textures=[gradient_texture()]), W, H, max_depth=depth, flags=flags)
    r0.render(frt.CameraController().build_uniform(W / H, 0, fresh.num_lights))
    rf.clear(); rf.render(frt.CameraController().build_uniform(W / H, 0, fresh.num_lights))
    assert r0.read_buffer(frt.BUF_GALBEDO, 0).tobytes() != rf.read_buffer(frt.BUF_GALBEDO, 0).tobytes()
    assert r0.read_accum().tobytes() != rf.read_accum().tobytes()


def test_mid_sequence_edit_with_the_pipeline(gpu):
    """Render 3 frames, edit, render 3 more: the two-stream schedule (whose next frame's G-buffer + T-trace ran ahead under the old values) equals the
    one-stream schedule on every buffer of every frame. As in test_instance_update_gpu.py::test_mid_sequence_move_with_the_pipeline, with two G-buffer
    sets the frame running ahead writes the set of the previous logical slot, so only the frame's own slot of the G-buffer targets is compared."""
    frt = gpu
    W, H = 96, 64
    fs = cornell_look(frt, color_textures=[gradient_texture()])
    edit = cornell_edit(frt)
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(6):
        if f == 3:
            apply_edit(a, edit); apply_edit(b, edit)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        for buf in range(8):
            for idx in ((0, 1) if buf in (0, 1, 2, 4, 7) else (0,)):
                if buf in (0, 1, 2) and idx != f % 2:
                    continue
                g, w = b.read_buffer(buf, idx), a.read_buffer(buf, idx)
                assert g.tobytes() == w.tobytes(), f"frame {f} buffer {buf}[{idx}]"
    sa, sb = a.stats(), b.stats()
    assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    assert sb["discarded_speculations"] >= 1          # the frame speculated under the old values was dropped


def test_queries_see_a_new_instance_material(gpu):
    frt = gpu
    W, H = 64, 48
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cams = [frt.CameraController().build_uniform(W / H, f, fs.num_lights) for f in range(2)]
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1)
    h = r.pick(cams[0], xy)
    on_box = np.flatnonzero(h["instance"] == TALL_BOX)
    assert on_box.size > 20 and (h["material"][on_box] == METAL).all()
    r.render(cams[0])
    r.set_instance_materials([TALL_BOX], [RED])
    h = r.pick(cams[1], xy)
    assert (h["material"][on_box] == RED).all() and (h["instance"][on_box] == TALL_BOX).all()
    assert (h["material"][h["instance"] == CRYSTAL] == GLASS).all()
    origin = np.array([0.0, 0.0, 3.0], np.float32)
    p = on_box[on_box.size // 2]
    t = r.trace_closest(origin[None, :], np.array([[-0.35, -0.4, -0.3]], np.float32) - origin, 0.0, 2.0)      # towards the box's centre
    assert t["instance"][0] == TALL_BOX and t["material"][0] == RED
    r.render(cams[1])
    gpos = r.read_buffer(frt.BUF_GPOS, 1).view(np.float32).reshape(H * W, 4)      # frame 1's own slot
    assert (gpos[on_box, 3] == float(RED)).all() and gpos[p, 3] == float(RED)
    assert (gpos[:, 3] == h["material"].astype(np.float32))[h["tri"] != 0xFFFFFFFF].all()


def test_a_moved_light_keeps_its_new_emission(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    tree = {w: r.read_scene(w).tobytes() for w in TREE}
    r.render(frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights))
    both(r, fs, "set_light_emission", 1, (0.1, 0.9, 0.2), 7.0)
    both(r, fs, "set_light_emission", 0, (0.9, 0.8, 0.7), 4.0)
    both(r, fs, "set_instance_materials", [TALL_BOX], [GREEN])
    moves = cornell_moves(frt)
    ids = [SPHERE_LIGHT, QUAD_LIGHT, TALL_BOX]
    both(r, fs, "set_instance_transforms", ids, np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids]))
    for w in LOOK + TREE:
        assert r.read_scene(w).tobytes() == fs.get(w).tobytes(), w      # (a moved instance's device record is made again: it carries the new material)
    assert r.read_scene("lights").view(np.float32)[1, 12:16].tolist() == [np.float32(0.1), np.float32(0.9), np.float32(0.2), 7.0]
    assert r.read_scene("tri_slots").tobytes() != tree["tri_slots"]


def test_multi_renderer_strips_match_one_renderer(gpu):
    frt = gpu
    W, H = 64, 48
    fs = cornell_look(frt, color_textures=[gradient_texture()])
    edit = cornell_edit(frt)
    multi = frt.MultiRenderer(fs, W, H, [0, 0])
    one = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(4):
        if f == 2:
            apply_edit(multi, edit); apply_edit(one, edit)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        multi.render(cam); one.render(cam)
        if f >= 2:
            multi.sync()
            for buf in range(8):
                for idx in ((0, 1) if buf in (0, 1, 2, 4, 7) else (0,)):
                    if buf in (0, 1, 2) and idx != f % 2:      # (the G-buffer set a frame running ahead writes: see the mid-sequence test)
                        continue
                    assert multi.read_buffer(buf, idx).tobytes() == one.read_buffer(buf, idx).tobytes(), f"frame {f} buffer {buf}[{idx}]"
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    assert multi.read_display().tobytes() == one.read_display().tobytes()
    with pytest.raises(frt.FrtError):
        multi.set_instance_materials([SPHERE_LIGHT], [RED])
    with pytest.raises(frt.FrtError):
        multi.set_texture("color", 4, edit[3])


def test_renderer_argument_and_state_errors(gpu):
    frt = gpu
    L = frt.lib()
    fs = cornell_look(frt, color_textures=[gradient_texture()])
    r = frt.Renderer(fs, 32, 32)
    what = LOOK + TREE
    before = {w: r.read_scene(w).tobytes() for w in what}
    ok = material(frt, [0.5, 0.5, 0.5, 1.0])
    no_layer = material(frt, [0.5, 0.5, 0.5, 1.0], texture=4)
    no_light = material(frt, [0.5, 0.5, 0.5, 1.0]); no_light.light_index = 2
    tex = checker_texture(16)
    refused = [
        lambda: r.set_materials([8], [ok]), lambda: r.set_materials([0, 8], [ok, ok]), lambda: r.set_materials([0, 1], [ok, no_layer]),
        lambda: r.set_materials([0, 2], [ok, no_light]),
        lambda: r.set_instance_materials([9], [0]), lambda: r.set_instance_materials([TALL_BOX, 0], [RED, 8]),
        lambda: r.set_instance_materials([TALL_BOX, SPHERE_LIGHT], [RED, RED]), lambda: r.set_instance_materials([QUAD_LIGHT], [RED]),
        lambda: r.set_light_emission(2, (1, 1, 1), 1.0),
        lambda: r.set_texture("color", 4, tex), lambda: r.set_texture("data", 3, tex), lambda: r.set_texture(2, 0, tex),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(frt.FrtError):
            call()
        assert L.frt_last_error() != b""
    ids = np.array([0], np.uint32)
    assert L.frt_renderer_set_materials(r._h, 1, ids.ctypes.data, None) == -1                # FRT_ERR_INVALID_ARG
    assert L.frt_renderer_set_instance_materials(r._h, 1, None, ids.ctypes.data) == -1
    assert L.frt_renderer_set_light_emission(r._h, 0, None, 1.0) == -1
    assert L.frt_renderer_set_texture(r._h, 0, 0, None) == -1
    assert L.frt_renderer_set_materials(None, 0, None, None) == -1
    assert L.frt_renderer_set_materials(r._h, 0, None, None) == 0 and L.frt_renderer_set_instance_materials(r._h, 0, None, None) == 0
    assert {w: r.read_scene(w).tobytes() for w in what} == before                             # the replica is unchanged
    cam = frt.CameraController().build_uniform(1.0, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    c = np.ones(3, np.float32)
    one = np.array([TALL_BOX], np.uint32); red = np.array([RED], np.uint32)
    assert L.frt_renderer_set_materials(r._h, 1, ids.ctypes.data, np.frombuffer(bytes(ok), np.uint8).ctypes.data) == -4      # FRT_ERR_STATE: a frame is open
    assert L.frt_renderer_set_instance_materials(r._h, 1, one.ctypes.data, red.ctypes.data) == -4
    assert L.frt_renderer_set_light_emission(r._h, 0, c.ctypes.data, 1.0) == -4
    assert L.frt_renderer_set_texture(r._h, 0, 3, tex.ctypes.data) == -4
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    assert {w: r.read_scene(w).tobytes() for w in what} == before
    both(r, fs, "set_materials", [0], [ok]); both(r, fs, "set_instance_materials", [TALL_BOX], [RED])      # between frames they are taken
    both(r, fs, "set_light_emission", 0, (1, 1, 1), 1.0); both(r, fs, "set_texture", "color", 3, tex)
    assert_replica(r, fs, {w: before[w] for w in TREE}, "after the open frame")
