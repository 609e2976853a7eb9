"""Removing materials, meshes, lights and texture layers on the device (include/frt.h: frt_renderer_remove_materials and the three calls after it; DESIGN.md
section 16). As everywhere since section 14 every comparison is bit equality: of the replica's records with the scene built from scratch with the surviving
builder calls, of every buffer of every frame with a renderer over that scene and with the brute-force oracle over it, and of the per-pixel history with
what numpy makes of it."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_instance_add_remove_gpu import check_replica, renderer, CONFIGS, BYTE_FOR_BYTE
from _instance_lists import cornell_list, one_triangle, trs
from _scene_remove_lists import Calls, rich, solid_layer, stripes_layer

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = -1, -4
POOLS = ("attributes", "indices", "mesh_infos")      # selectors 4 - 6
MODE = {"morton": 1, "sah": 2}
GLASS, CRYSTAL_INSTANCE = 5, 6      # rich(): material 5 is used by instance 6 alone
PIXEL_BUFFERS = [("GPOS", 0), ("GPOS", 1), ("GNORMAL", 0), ("GNORMAL", 1), ("GALBEDO", 0), ("GALBEDO", 1), ("GMOTION", 0), ("RESERVOIR", 0), ("RESERVOIR", 1), ("RAW", 0), ("DISPLAY", 0),
                 ("ACCUM", 0), ("ACCUM", 1), ("CANDIDATE", 0)]


def oracle_scene(orc, fs, calls):
    """The oracle's own scene from the product scene's materials, lights and instances and the calls' meshes and texture layers (nothing of any tree)."""
    from _oracle import OrcScene
    oh = orc.L.orc_scene_create()
    for g in calls.meshes:
        pos = np.ascontiguousarray(g.positions, np.float32); att = np.ascontiguousarray(g.attributes, np.float32); idx = np.ascontiguousarray(g.indices, np.uint32)
        orc.L.orc_scene_add_mesh(oh, pos.ctypes.data, pos.shape[0], att.ctypes.data, idx.ctypes.data, idx.size)
    for c in calls.calls:
        if c["kind"] in ("ctex", "dtex"):
            px = np.ascontiguousarray(c["px"], np.uint8)
            orc.L.orc_scene_add_texture(oh, 0 if c["kind"] == "ctex" else 1, px.ctypes.data)
    for row in fs.get("materials"):
        r = np.ascontiguousarray(row); orc.L.orc_scene_add_material(oh, r.ctypes.data)
    for row in fs.get("lights"):
        r = np.ascontiguousarray(row); orc.L.orc_scene_add_light(oh, r.ctypes.data)
    for row in fs.get("instances"):
        m = np.ascontiguousarray(row[5:21]); orc.L.orc_scene_add_instance(oh, int(row[0]), int(row[1]), m.ctypes.data)
    orc.L.orc_scene_build(oh)
    return OrcScene(orc, oh)


def check_all(frt, r, fresh, what, origin):
    check_replica(frt, r, fresh, what, origin=origin)
    n = fresh.counts()
    p = r.pool_counts()
    assert (p["meshes"], p["vertices"], p["indices"]) == (n["meshes"], n["attributes"], n["indices"]), what
    for w in POOLS:
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), f"{what}: {w}"


def check_frames(frt, orc, r, calls, fresh, cfg, what, frames=2, oracle=True):
    """`r` from a cleared state against a renderer over `fresh` and the brute-force oracle over it: every buffer of every frame, and the ray counts."""
    flags, W, H = CONFIGS[cfg]
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=8, flags=flags)
    ro = oracle_scene(orc, fresh, calls).renderer(W, H, 8, False, 16) if oracle else None
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        for x in (r, rf) + ((ro,) if oracle else ()):
            x.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, f"{what}: edited vs fresh build")
        if oracle:
            compare_all(r.read_buffer, ro.read, f, f"{what}: edited vs brute-force oracle")
    st, sf = r.stats(), rf.stats()
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"]), what
    if oracle:
        so = ro.stats()["total"]
        assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"]), what


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_materials(gpu, orc, cfg):
    frt = gpu
    calls = rich(frt)
    r = renderer(frt, calls.build(frt), cfg)
    r.remove_materials([8, 6, 8])      # the last unregistered one and a middle one, one of them twice: the lamps' 9 and 10 and the textured 7 shift down
    calls = calls.without_materials([6, 8])
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "materials 6 and 8", origin=0)
    check_frames(frt, orc, r, calls, fresh, cfg, f"materials 6 and 8, {cfg}", oracle=cfg == "one stream")
    r.remove_instances([3], quality="morton")      # the red wall, then the first material
    r.remove_materials(0)
    calls = calls.without_instances([3]).without_materials([0])
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "material 0", origin=1)
    check_frames(frt, orc, r, calls, fresh, cfg, f"material 0, {cfg}", oracle=cfg == "pipeline")


def test_meshes(gpu, orc):
    frt = gpu
    cfg = "one stream"
    calls = rich(frt)
    r = renderer(frt, calls.build(frt), cfg)
    assert r.add_meshes(frt.geometry.create_crystal()) == 5
    r.remove_instances([0, 1, 2, 3, 4], quality="sah")      # every user of mesh 0 (the plane): the walls ...
    r.remove_lights([2], quality="sah")                      # ... and the quad lamp
    r.remove_meshes(0)                                       # every offset shifts
    r.remove_meshes([4, 4])                                  # the mesh that came from add_meshes (5, now 4)
    calls = calls.without_instances([0, 1, 2, 3, 4]).without_lights([2]).without_meshes([0])
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "meshes 0 and the added one", origin=2)
    check_frames(frt, orc, r, calls, fresh, cfg, "meshes 0 and the added one", oracle=False)
    # the renumbered meshes take the other edits: the cube is 0 now, the one-triangle mesh 3
    cube = frt.geometry.create_cube()
    pos = np.array(cube.positions, np.float32); pos[:, 0] *= 1.0 + 0.3 * pos[:, 1]
    att = np.array(cube.attributes, np.float32); att[:, 2:4] = att[:, 2:4] * 0.5 + 0.25
    m = trs(frt, (-0.3, 0.35, 0.3), 0.5, 0.4)
    r.set_mesh_vertices(0, pos, att)
    n = r.scene_counts()["instances"]
    assert r.add_instances(3, 1, m) == n
    made = calls._made_by(("mesh",))
    calls.calls[made[0]]["geo"] = frt.geometry.Geometry(pos, att, cube.indices)
    calls = calls.plus({"kind": "inst", "mesh": 3, "mat": 1, "m": m})
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "edits on renumbered meshes", origin=None)
    check_frames(frt, orc, r, calls, fresh, cfg, "edits on renumbered meshes")


@pytest.mark.parametrize("cfg,quality", [("one stream", "sah"), ("pipeline", "morton")])
def test_lights(gpu, orc, cfg, quality):
    frt = gpu
    calls = rich(frt)      # lights: 0 and 1 of add_light (material 7 names 1), 2 the registered quad, 3 the registered sphere
    r = renderer(frt, calls.build(frt), cfg)
    r.remove_lights(0, quality=quality)
    calls = calls.without_lights([0])
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "an add_light light", origin=0)      # (no triangle work: still the host build's tree)
    check_frames(frt, orc, r, calls, fresh, cfg, f"an add_light light, {cfg}", oracle=False)
    r.remove_lights([1, 1], quality=quality)      # the quad lamp: its record, its instance (5) and its material (9)
    calls = calls.without_lights([1])
    fresh = calls.build(frt)
    assert r.scene_counts() == {"tris": fresh.counts()["tris"], "instances": 9, "materials": 10, "lights": 2}
    check_all(frt, r, fresh, "the quad lamp", origin=MODE[quality])
    # the sphere lamp is instance 6 and light 1 now: it still moves its light record, and takes set_light_emission under the new index
    moved = trs(frt, (0.3, -0.4, 0.4), 0.12)
    for x in (r, fresh):
        x.set_instance_transforms([6], [moved])
        x.set_light_emission(1, (0.9, 0.3, 0.1), 6.0)
    for w in BYTE_FOR_BYTE:
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), f"after the move and the emission edit: {w}"
    made = calls._made_by(("inst", "quad", "sphere"))
    calls.calls[made[6]].update(m=moved, color=(0.9, 0.3, 0.1), intensity=6.0)
    check_frames(frt, orc, r, calls, calls.build(frt), cfg, f"the quad lamp, {cfg}", oracle=cfg == "one stream")
    other = "morton" if quality == "sah" else "sah"
    r.remove_lights(1, quality=other)      # the sphere lamp in the other mode
    calls = calls.without_lights([1])
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "the sphere lamp", origin=MODE[other])
    check_frames(frt, orc, r, calls, fresh, cfg, f"the sphere lamp, {cfg}", oracle=cfg == "pipeline")


def test_textures(gpu, orc):
    frt = gpu
    cfg = "one stream"
    calls = rich(frt)
    made = calls._made_by(("ctex",)) + calls._made_by(("dtex",))      # a pattern in the layers the visible material 7 names (colour 4, data 4): a wrong layer shows
    calls.calls[made[1]]["px"] = stripes_layer(32, (250, 250, 30, 255), (30, 30, 250, 255))
    calls.calls[made[3]]["px"] = stripes_layer(64, (255, 40, 230, 255), (255, 220, 20, 255))
    r = renderer(frt, calls.build(frt), cfg)
    r.remove_texture("color", 3)
    r.remove_texture("data", 3)
    calls = calls.without_texture(0, 3).without_texture(1, 3)
    fresh = calls.build(frt)
    check_all(frt, r, fresh, "layer 3 of both kinds", origin=0)
    p = r.pool_counts()
    assert (p["color_layers"], p["data_layers"]) == (4, 4)
    check_frames(frt, orc, r, calls, fresh, cfg, "layer 3 of both kinds")
    assert r.add_texture("color", solid_layer((9, 9, 9, 255))) == 4      # the count moved, the room stayed
    assert r.pool_counts()["growths"] == 0


def remapped(frt, gpos, mat_map):
    """What the library makes of a G-buffer set's position texels under an old -> new material table (-1: the material left)."""
    out = gpos.copy().view(np.float32)
    w = out[..., 3]
    hit = w >= 0
    ids = (w[hit] + np.float32(0.1)).astype(np.uint32)
    new = np.array([mat_map.get(int(i), -1) for i in ids], np.int64)
    w[hit] = np.where(new < 0, np.float32(65535.0), new.astype(np.float32))
    return out.view(np.uint8)


def pixel_state(frt, r, skip=()):
    return {(b, i): r.read_buffer(getattr(frt, "BUF_" + b), i).tobytes() for b, i in PIXEL_BUFFERS if b not in skip}


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_history_remap(gpu, cfg):
    frt = gpu
    calls = rich(frt)
    r = renderer(frt, calls.build(frt), cfg)
    before = pixel_state(frt, r)
    gpos = [r.read_buffer(frt.BUF_GPOS, i) for i in (0, 1)]
    seen = set(np.unique(gpos[0].view(np.float32)[..., 3]).tolist()) | set(np.unique(gpos[1].view(np.float32)[..., 3]).tolist())
    assert float(GLASS) in seen and 7.0 in seen and 9.0 in seen      # the glass crystal, the textured box and the quad lamp are on screen
    fc = r.frame_count
    r.remove_instances(CRYSTAL_INSTANCE)
    r.remove_materials(GLASS)      # no frame in between
    mat_map = calls.material_map([GLASS])
    after = pixel_state(frt, r)
    for i in (0, 1):
        want = remapped(frt, gpos[i], mat_map)
        assert after[("GPOS", i)] == want.tobytes(), f"GPOS[{i}]"
        w = want.view(np.float32)[..., 3]
        assert (w == 65535.0).any() and (w == 8.0).any() and (w == 6.0).any()      # gone; the quad lamp's 9 and the textured box's 7, one down
    for k in before:
        if k[0] != "GPOS":
            assert after[k] == before[k], k
    assert r.frame_count == fc
    # a second removal leaves 65535 alone
    r.remove_materials(5)      # (the unused material that was 6)
    again = r.read_buffer(frt.BUF_GPOS, 0).view(np.float32)[..., 3]
    assert (again == 65535.0).sum() == (remapped(frt, gpos[0], mat_map).view(np.float32)[..., 3] == 65535.0).sum() and (again == 7.0).any()


def test_history_continues(gpu):
    """An edited renderer that is not cleared goes on exactly as a renderer over the scratch build that was handed its per-pixel buffers."""
    frt = gpu
    cfg = "one stream"
    flags, W, H = CONFIGS[cfg]
    calls = rich(frt)
    a = renderer(frt, calls.build(frt), cfg)
    a.remove_instances(CRYSTAL_INSTANCE)
    a.remove_materials([GLASS, 6])
    a.remove_lights(0)
    calls = calls.without_instances([CRYSTAL_INSTANCE]).without_materials([GLASS, 6]).without_lights([0])
    fresh = calls.build(frt)
    b = renderer(frt, fresh, cfg)      # as many frames as `a`
    assert a.frame_count == b.frame_count == 2
    for name, i in PIXEL_BUFFERS:
        buf = getattr(frt, "BUF_" + name)
        b.write_rows(buf, i, 0, H, a.read_buffer(buf, i))
    for f in (2, 3):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        a.render(cam); b.render(cam)
        compare_all(a.read_buffer, b.read_buffer, f, "edited and not cleared vs scratch build with the same history")
        for name, i in PIXEL_BUFFERS:
            buf = getattr(frt, "BUF_" + name)
            assert a.read_buffer(buf, i).tobytes() == b.read_buffer(buf, i).tobytes(), (f, name, i)


def test_round_trip(gpu, orc):
    frt = gpu
    cfg = "pipeline"
    lst = cornell_list(frt)
    first = lst.build(frt)
    r = renderer(frt, lst.build(frt), cfg)
    m = trs(frt, (-0.3, 0.35, 0.3), 0.5, 0.4)
    assert r.add_texture("color", solid_layer((200, 30, 30, 255))) == 3
    mat = frt.material_new([0.9, 0.9, 0.9, 1.0]); mat.tex_info_0 = 3 | (0xFFFF << 16)
    assert r.add_materials(mat) == 8 and r.add_meshes(frt.geometry.create_crystal()) == 5
    assert r.add_instances(5, 8, m) == 9
    assert r.register_quad_light(0, trs(frt, (0.4, 0.6, 0.2), 0.3, 0.2), (1.0, 0.8, 0.6), 4.0) == 2
    r.render(frt.CameraController().build_uniform(CONFIGS[cfg][1] / CONFIGS[cfg][2], 2, 3))
    r.remove_lights(2); r.remove_instances(9); r.remove_meshes(5); r.remove_materials(8); r.remove_texture("color", 3)
    for w in ("materials", "lights", "instances_dev", "shade_tris") + POOLS:
        assert r.read_scene(w).tobytes() == first.get(w).tobytes(), w
    assert r.pool_counts()["color_layers"] == 3
    from test_instance_add_remove_gpu import check_frames as frames_of_list
    frames_of_list(frt, orc, r, lst, first, cfg, "round trip", frames=3, oracle=False)


def decoded_normals(frt, attrs):
    """What the host's decoded_vertex_normal makes of the attribute records `attrs`, (xyz, 0) per vertex: host_normals over one mesh that holds them (a
    shading record's normals do not depend on the positions)."""
    from test_scene_grow_gpu import host_normals
    n = len(attrs)
    v = np.arange(n, dtype=np.float32)
    pos = np.stack([np.cos(v), np.sin(v), 0.01 * v, np.ones(n, np.float32)], axis=1).astype(np.float32)
    return host_normals(frt, [frt.geometry.Geometry(pos, np.ascontiguousarray(attrs, np.float32).reshape(n, 8), np.arange(3, dtype=np.uint32))])


def test_capacities_across_edit_families(gpu):
    """One renderer through the orders in which the capacities of the edit families hand over to each other: a removal on pools that never grew, growth from
    the pinned capacities, a deformation and a rebuild on the grown buffers, removal again (spares smaller than their pools), and an addition that fits."""
    from test_scene_grow_gpu import pyramid, new_materials, new_transforms
    frt = gpu
    cfg = "pipeline"
    lst = cornell_list(frt)
    lst.materials.append(frt.material_new([0.1, 0.2, 0.3, 1.0]))      # 6: no instance uses it (the registered lights' materials are 7 and 8 then)
    calls = Calls.of_list(lst)
    r = renderer(frt, calls.build(frt), cfg)

    def check(what, origin):
        fresh = calls.build(frt)
        check_all(frt, r, fresh, what, origin=origin)
        assert r.read_scene("normals").tobytes() == decoded_normals(frt, r.read_scene("attributes")).tobytes(), f"{what}: normals"
        return fresh

    # 1. removal first: the pools are pinned at their counts
    r.remove_materials(6)
    r.remove_meshes(4)      # the one-triangle mesh
    calls = calls.without_materials([6]).without_meshes([4])
    assert r.pool_counts()["growths"] == 0
    # 2. growth from a pinned capacity
    me, ma, m = [4, 4, 4], [8, 9, 8], new_transforms(frt)
    light = {"kind": "quad", "mesh": 0, "m": trs(frt, (0.4, 0.6, 0.2), 0.3, 0.2), "color": (1.0, 0.8, 0.6), "intensity": 4.0}
    assert r.add_meshes([frt.geometry.create_sphere(1), pyramid(frt)]) == 4      # (more vertices than the 3 the removed mesh left room for)
    assert r.add_materials(new_materials(frt)) == 8
    assert r.add_instances(me, ma, m) == 9
    assert r.register_quad_light(light["mesh"], light["m"], light["color"], light["intensity"]) == 2
    assert r.pool_counts()["growths"] >= 1
    calls = calls.plus({"kind": "mesh", "geo": frt.geometry.create_sphere(1)}, {"kind": "mesh", "geo": pyramid(frt)}, *[{"kind": "material", "mat": x} for x in new_materials(frt)],
                       *[{"kind": "inst", "mesh": a, "mat": b, "m": c} for a, b, c in zip(me, ma, m)], light)
    check("growth from a pinned capacity", origin=2)
    # 3. a mesh from before step 1 deformed (its decoded normals live in a grown, once-compacted buffer), then a rebuild
    cube = frt.geometry.create_cube()
    pos = np.array(cube.positions, np.float32); pos[:, 0] *= 1.0 + 0.3 * pos[:, 1]
    att = np.array(cube.attributes, np.float32); att[:, 2:4] = att[:, 2:4] * 0.5 + 0.25
    att[:, 0:2] = att[::-1, 0:2].copy()      # (other normals too: valid encodings, each another vertex's)
    r.set_mesh_vertices(1, pos, att)
    r.rebuild_tree(quality="sah")
    calls.calls[calls._made_by(("mesh",))[1]]["geo"] = frt.geometry.Geometry(pos, att, cube.indices)
    # 4. removal again: the light of step 2, two of its instances, its unused mesh (whose spares are smaller than the pools by now)
    r.remove_lights(2)
    r.remove_instances([10, 11])
    r.remove_meshes(5)
    calls = calls.without_lights([2]).without_instances([10, 11]).without_meshes([5])
    check("removal after growth", origin=2)
    # 5. step 2's instances once more: they fit
    growths = r.pool_counts()["growths"]
    assert r.add_instances(me, ma, m) == 10
    assert r.pool_counts()["growths"] == growths
    calls = calls.plus(*[{"kind": "inst", "mesh": a, "mat": b, "m": c} for a, b, c in zip(me, ma, m)])
    fresh = check("an addition that fits", origin=2)
    check_frames(frt, None, r, calls, fresh, cfg, "capacities across the edit families", frames=2, oracle=False)


def test_refusals_change_nothing(gpu):
    frt = gpu
    L = frt.lib()
    flags, W, H = CONFIGS["pipeline"]
    calls = rich(frt)
    r, twin = renderer(frt, calls.build(frt), "pipeline"), renderer(frt, calls.build(frt), "pipeline")
    what = BYTE_FOR_BYTE + POOLS + ("tri_slots", "quad_nodes")
    state = lambda x: ({w: x.read_scene(w).tobytes() for w in what}, x.tree_stats(), x.scene_counts(), x.pool_counts(), x.frame_count)
    u32 = lambda *v: np.asarray(v, np.uint32)
    ids = lambda name, v, *mode: getattr(L, "frt_renderer_" + name)(r._h, len(v), v.ctypes.data, *mode)
    assert ids("remove_materials", u32(6, 2)) == ERR_INVALID_ARG and b"still uses" in L.frt_last_error()                     # in use
    assert ids("remove_materials", u32(10)) == ERR_INVALID_ARG and b"remove the light" in L.frt_last_error()                  # a registered light's material
    assert ids("remove_materials", u32(11)) == ERR_INVALID_ARG and ids("remove_meshes", u32(5)) == ERR_INVALID_ARG and ids("remove_lights", u32(4), 1) == ERR_INVALID_ARG
    assert ids("remove_meshes", u32(4, 0)) == ERR_INVALID_ARG and ids("remove_lights", u32(0, 1), 1) == ERR_INVALID_ARG      # in use; named by material 7
    assert ids("remove_lights", u32(0), 2) == ERR_INVALID_ARG and b"rebuild mode" in L.frt_last_error()                        # an unknown rebuild mode
    tex = lambda kind, layer: L.frt_renderer_remove_texture(r._h, kind, layer)
    assert tex(0, 4) == ERR_INVALID_ARG and tex(1, 4) == ERR_INVALID_ARG and tex(0, 0) == ERR_INVALID_ARG and tex(1, 2) == ERR_INVALID_ARG      # in use; builder-default layers
    assert tex(0, 5) == ERR_INVALID_ARG and tex(2, 3) == ERR_INVALID_ARG
    for name in ("remove_materials", "remove_meshes"):
        assert getattr(L, "frt_renderer_" + name)(r._h, 1, None) == ERR_INVALID_ARG and getattr(L, "frt_renderer_" + name)(r._h, 0, None) == 0
    assert L.frt_renderer_remove_lights(r._h, 1, None, 0) == ERR_INVALID_ARG and L.frt_renderer_remove_lights(r._h, 0, None, 1) == 0
    cam = frt.CameraController().build_uniform(W / H, 2, 4)
    for x in (r, twin):
        x.render_phases(cam, frt.PHASE_GBUFFER)
    assert ids("remove_materials", u32(6)) == ERR_STATE and ids("remove_meshes", u32(4)) == ERR_STATE and ids("remove_lights", u32(0), 1) == ERR_STATE and tex(0, 3) == ERR_STATE
    assert b"frame is open" in L.frt_last_error()
    for x in (r, twin):
        x.render_phases(cam, frt.PHASE_ALL); x.end_frame()
    assert state(r) == state(twin)
    assert pixel_state(frt, r) == pixel_state(frt, twin)
    cam = frt.CameraController().build_uniform(W / H, 3, 4)
    r.render(cam); twin.render(cam)
    compare_all(r.read_buffer, twin.read_buffer, 3, "the frame after the refusals")


def test_multi_renderer(gpu):
    frt = gpu
    flags, W, H = CONFIGS["pipeline"]
    calls = rich(frt)
    one = frt.Renderer(calls.build(frt), W, H, max_depth=8, flags=flags)
    two = frt.MultiRenderer(calls.build(frt), W, H, [0, 0], max_depth=8, flags=flags)

    def frames(lo, hi, lights):
        for f in range(lo, hi):
            cam = frt.CameraController().build_uniform(W / H, f, lights)
            one.render(cam); two.render(cam)
            for b, idx in ((frt.BUF_ACCUM, 0), (frt.BUF_ACCUM, 1), (frt.BUF_DISPLAY, 0), (frt.BUF_RAW, 0), (frt.BUF_RESERVOIR, 0), (frt.BUF_RESERVOIR, 1)):
                assert one.read_buffer(b, idx).tobytes() == two.read_buffer(b, idx).tobytes(), f"frame {f}, buffer {b}[{idx}]"

    frames(0, 2, 4)
    for x in (one, two):
        x.remove_instances(CRYSTAL_INSTANCE); x.remove_materials([GLASS, 6]); x.remove_meshes(4); x.remove_lights([0, 2], quality="morton"); x.remove_texture("data", 3)
    frames(2, 5, 2)
    fresh = calls.without_instances([CRYSTAL_INSTANCE]).without_materials([GLASS, 6]).without_meshes([4]).without_lights([0, 2]).without_texture(1, 3).build(frt)
    for w in BYTE_FOR_BYTE + POOLS:
        assert one.read_scene(w).tobytes() == fresh.get(w).tobytes(), w
