"""Editing what a built scene looks like (include/frt.h: frt_scene_set_materials, _set_instance_materials, _set_light_emission, _set_texture;
DESIGN.md section 13), on the host: after any sequence of the four edits the scene equals one built from scratch with the edited values, no
triangle, slot or box moves, a refused call changes nothing, and build() still rejects what it rejected through the now shared material check."""
import ctypes as C
import numpy as np
import pytest
from test_instance_update import cornell_meshes, cornell_moves, by_id, QUAD_LIGHT, CRYSTAL, SPHERE_LIGHT, TALL_BOX

# Cornell Box materials (scenes.rs:20-48 order): 0 red, 1 green, 2 white, 3 checker, 4 metal, 5 glass; 6 and 7 are made by the two register_*_light calls
RED, GREEN, WHITE, CHECKER, METAL, GLASS, QUAD_LIGHT_MAT, SPHERE_LIGHT_MAT = range(8)
FLOOR = 0
LOOK = ("materials", "lights", "instances_dev", "shade_tris", "instances")      # what the edits may change
FIXED = ("tris", "tri_slots", "quad_nodes")                                      # what they never touch
CORNELL_EMISSION = {0: ((1.0, 1.0, 1.0), 10.0), 1: ((0.02, 0.02, 0.9), 10.0)}    # scenes.rs:92, :112


def material(frt, rgba, roughness=None, texture=None, metallic=None):
    m = frt.material_new(rgba)
    if roughness is not None:
        m.roughness = roughness
    if metallic is not None:
        m.metallic = metallic
    if texture is not None:
        m.tex_info_0 = (m.tex_info_0 & 0xFFFF0000) | texture
    return m


def checker_texture(period):
    y, x = np.mgrid[0:1024, 0:1024]
    on = ((x // period + y // period) % 2 == 0)
    t = np.zeros((1024, 1024, 4), np.uint8)
    t[..., 0] = np.where(on, 230, 20); t[..., 1] = np.where(on, 200, 40); t[..., 2] = np.where(on, 40, 160); t[..., 3] = 255
    return t


def gradient_texture():
    y, x = np.mgrid[0:1024, 0:1024]
    t = np.zeros((1024, 1024, 4), np.uint8)
    t[..., 0] = x // 4; t[..., 1] = y // 4; t[..., 2] = 128; t[..., 3] = 255
    return t


def cornell_look(frt, materials=None, inst_mats=None, emissions=None, moves=None, color_textures=()):
    """The Cornell Box of scenes.rs issued call by call through the public builder, from scratch: material k = materials[k], instance k with material
    inst_mats[k] and transform moves[k], light k registered with emissions[k] = (colour, intensity), where given; color_textures become layers 3, 4, ..."""
    materials, inst_mats, emissions, moves = materials or {}, inst_mats or {}, {**CORNELL_EMISSION, **(emissions or {})}, moves or {}
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    b = frt.SceneBuilder()
    for t in color_textures:
        b.add_color_texture(t)
    for g in cornell_meshes(frt):
        b.add_mesh(g)
    for k in range(6):
        b.add_material(materials[k] if k in materials else frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()))
    for k, row in enumerate(inst):
        m = np.asarray(moves[k], np.float32).reshape(16) if k in moves else row[5:21].view(np.float32)
        if k == QUAD_LIGHT:
            b.register_quad_light(int(row[0]), m, *emissions[0])
        elif k == SPHERE_LIGHT:
            b.register_sphere_light(int(row[0]), m, *emissions[1])
        else:
            b.add_instance(int(row[0]), inst_mats.get(k, int(row[1])), m)
    return b.build()


def restir_look(frt, materials=None, inst_mats=None, emissions=None):
    """The ReSTIR scene of scenes.rs from scratch, through the public builder, with the same overrides (its lights are add_light's: no instance link)."""
    materials, inst_mats, emissions = materials or {}, inst_mats or {}, emissions or {}
    ref = frt.scenes.create_restir_scene()
    g = frt.geometry
    b = frt.SceneBuilder()
    for geo in (g.create_plane(), g.create_sphere(2), g.create_cube()):
        b.add_mesh(geo)
    for k, row in enumerate(ref.get("materials")):
        b.add_material(materials[k] if k in materials else frt.Material.from_buffer_copy(np.ascontiguousarray(row).tobytes()))
    for k, row in enumerate(ref.get("lights")):
        l = frt.Light.from_buffer_copy(np.ascontiguousarray(row).tobytes())
        if k in emissions:
            l.emission[:] = list(emissions[k][0]) + [emissions[k][1]]
        b.add_light(l)
    for k, row in enumerate(ref.get("instances")):
        b.add_instance(int(row[0]), inst_mats.get(k, int(row[1])), row[5:21].view(np.float32))
    return b.build()


def snapshot(s, what=LOOK + FIXED):
    return {w: s.get(w).tobytes() for w in what}


def assert_equal_scenes(got, want, ctx):
    for w in LOOK:
        a, b = got.get(w), want.get(w)
        assert a.tobytes() == b.tobytes(), f"{ctx}: {w}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} words differ"


def cornell_edit(frt):
    """One edit of each kind, for the Cornell Box with a fourth colour layer: (materials, instance materials, emissions, the new layer 3)."""
    return ({METAL: material(frt, [0.2, 0.5, 0.9, 1.0], roughness=0.6, texture=3, metallic=0.0)}, {CRYSTAL: GREEN},
            {0: ((1.0, 1.0, 1.0), 5.0)}, checker_texture(128))


def apply_edit(target, edit):
    """The four edits on a SceneBuilder, a Renderer or a MultiRenderer (they share the method names)."""
    mats, inst_mats, emissions, layer3 = edit
    target.set_materials(sorted(mats), [mats[k] for k in sorted(mats)])
    target.set_instance_materials(sorted(inst_mats), [inst_mats[k] for k in sorted(inst_mats)])
    for light, (color, intensity) in sorted(emissions.items()):
        target.set_light_emission(light, color, intensity)
    target.set_texture("color", 3, layer3)


def test_from_scratch_builders_equal_the_factories(frt):
    for a, b in ((frt.scenes.create_cornell_box(), cornell_look(frt)), (frt.scenes.create_restir_scene(), restir_look(frt))):
        for w in LOOK + FIXED:
            assert a.get(w).tobytes() == b.get(w).tobytes(), w


def test_cornell_edit_sequence_equals_a_scene_built_from_scratch(frt):
    layers = [gradient_texture()]
    s = cornell_look(frt, color_textures=layers)
    before = snapshot(s, FIXED)
    blue, rough_white, final_metal = material(frt, [0.1, 0.2, 0.9, 1.0]), material(frt, [0.7, 0.7, 0.7, 1.0], roughness=0.9, texture=3), material(frt, [0.9, 0.6, 0.2, 1.0], metallic=1.0, roughness=0.3)
    s.set_materials([METAL, WHITE, METAL], [blue, rough_white, final_metal])                  # METAL twice: ends with its last value
    assert_equal_scenes(s, cornell_look(frt, {METAL: final_metal, WHITE: rough_white}, color_textures=layers), "set_materials")
    s.set_instance_materials([TALL_BOX, CRYSTAL, TALL_BOX, FLOOR], [RED, GREEN, CHECKER, WHITE])   # TALL_BOX twice
    assert_equal_scenes(s, cornell_look(frt, {METAL: final_metal, WHITE: rough_white}, {TALL_BOX: CHECKER, CRYSTAL: GREEN, FLOOR: WHITE}, color_textures=layers), "set_instance_materials")
    s.set_light_emission(0, (1.0, 0.9, 0.8), 5.0)
    s.set_light_emission(1, (0.9, 0.1, 0.3), 2.5)
    s.set_texture("color", 3, checker_texture(32)).set_texture("data", 1, gradient_texture())
    fresh = cornell_look(frt, {METAL: final_metal, WHITE: rough_white}, {TALL_BOX: CHECKER, CRYSTAL: GREEN, FLOOR: WHITE},
                         {0: ((1.0, 0.9, 0.8), 5.0), 1: ((0.9, 0.1, 0.3), 2.5)}, color_textures=[checker_texture(32)])
    assert_equal_scenes(s, fresh, "all four")
    m = s.get("materials").view(np.float32)
    assert m[QUAD_LIGHT_MAT, 4:7].tolist() == [np.float32(1.0) * np.float32(5.0), np.float32(0.9) * np.float32(5.0), np.float32(0.8) * np.float32(5.0)]
    assert s.get("shade_tris")[s.get("instances")[TALL_BOX, 2], 25].view(np.uint32) == CHECKER
    assert snapshot(s, FIXED) == before                                 # no triangle, slot or box moved
    # a second round on the edited scene, back to the factory's values: the factory's bytes
    orig = frt.scenes.create_cornell_box()
    om = orig.get("materials")
    s.set_materials([METAL, WHITE], [om[METAL], om[WHITE]])             # 64-byte rows are accepted as materials
    s.set_instance_materials([TALL_BOX, CRYSTAL, FLOOR], [METAL, GLASS, CHECKER])
    for light, (c, i) in CORNELL_EMISSION.items():
        s.set_light_emission(light, c, i)
    assert_equal_scenes(s, orig, "edited back")


def test_restir_edit_sequence_equals_a_scene_built_from_scratch(frt):
    s = frt.scenes.create_restir_scene()
    before = snapshot(s, FIXED)
    n_inst, n_mat = len(s.get("instances")), len(s.get("materials"))
    cube = n_inst - 1
    dim = frt.Material.from_buffer_copy(np.ascontiguousarray(s.get("materials")[20]).tobytes())      # a light sphere's material: keeps its light_index
    dim.emissive_factor[:] = [1.0, 2.0, 3.0]
    floor = material(frt, [0.3, 0.3, 0.35, 1.0], roughness=0.2, texture=1)
    s.set_materials([20, 0], [dim, floor])
    s.set_instance_materials([cube, 2, 50, 2], [1, 2, 0, n_mat - 1])
    mats_before_light = s.get("materials").tobytes()
    s.set_light_emission(17, (0.5, 0.25, 1.0), 40.0)
    assert s.get("materials").tobytes() == mats_before_light           # an add_light light has no material link: the record only
    assert_equal_scenes(s, restir_look(frt, {20: dim, 0: floor}, {cube: 1, 2: n_mat - 1, 50: 0}, {17: ((0.5, 0.25, 1.0), 40.0)}), "restir")
    assert snapshot(s, FIXED) == before


def test_emission_survives_a_move_of_the_lights_instance(frt):
    moves = {k: v for k, v in cornell_moves(frt).items() if k in (SPHERE_LIGHT, QUAD_LIGHT)}
    em = {0: ((0.9, 0.8, 0.7), 4.0), 1: ((0.1, 0.9, 0.2), 7.0)}
    s = frt.scenes.create_cornell_box()
    for light, (c, i) in em.items():
        s.set_light_emission(light, c, i)
    ids = sorted(moves)
    s.set_instance_transforms(ids, np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids]))
    fresh = cornell_look(frt, emissions=em, moves=moves)
    assert_equal_scenes(s, fresh, "emission, then move")
    assert s.get("tris").tobytes() == fresh.get("tris").tobytes()
    assert by_id(s.get("tri_slots")).tobytes() == by_id(fresh.get("tri_slots")).tobytes()
    assert s.get("lights").view(np.float32)[1, 12:16].tolist() == [np.float32(0.1), np.float32(0.9), np.float32(0.2), 7.0]


def test_empty_calls_are_ok(frt):
    s = frt.scenes.create_cornell_box()
    before = snapshot(s)
    L = frt.lib()
    assert L.frt_scene_set_materials(s._h, 0, None, None) == 0
    assert L.frt_scene_set_instance_materials(s._h, 0, None, None) == 0
    s.set_materials([], []).set_instance_materials([], [])
    assert snapshot(s) == before


def test_errors_change_nothing(frt):
    L = frt.lib()
    s = cornell_look(frt, color_textures=[gradient_texture()])         # 4 colour layers, 3 data layers, 8 materials, 2 lights, 9 instances
    before = snapshot(s)
    ok = material(frt, [0.5, 0.5, 0.5, 1.0])
    no_layer = material(frt, [0.5, 0.5, 0.5, 1.0], texture=4)           # base colour layer 4 of 4
    no_data_layer = material(frt, [0.5, 0.5, 0.5, 1.0]); no_data_layer.tex_info_2 = 0xFFFF0003      # metallic-roughness: data layer 3 of 3
    no_light = material(frt, [0.5, 0.5, 0.5, 1.0]); no_light.light_index = 2
    tex = gradient_texture()
    refused = [
        lambda: s.set_materials([8], [ok]),                             # id out of range
        lambda: s.set_materials([0, 8], [ok, ok]),                      # ... behind a valid one: nothing applied
        lambda: s.set_materials([0, 1], [ok, no_layer]),                # missing texture layer
        lambda: s.set_materials([1], [no_data_layer]),
        lambda: s.set_materials([0, 2], [ok, no_light]),                # light_index out of range
        lambda: s.set_materials([0, 1], [ok]),                          # one material for two ids
        lambda: s.set_instance_materials([9], [0]),                     # instance out of range
        lambda: s.set_instance_materials([TALL_BOX, 0], [RED, 8]),      # material out of range
        lambda: s.set_instance_materials([TALL_BOX, SPHERE_LIGHT], [RED, RED]),   # a registered light's instance
        lambda: s.set_instance_materials([QUAD_LIGHT], [QUAD_LIGHT_MAT]),
        lambda: s.set_instance_materials([0, 1], [0]),
        lambda: s.set_light_emission(2, (1, 1, 1), 1.0),                # light out of range
        lambda: s.set_light_emission(0, (1, 1), 1.0),
        lambda: s.set_texture("color", 4, tex),                         # wrong layer
        lambda: s.set_texture("data", 3, tex),
        lambda: s.set_texture(2, 0, tex),                               # wrong kind
        lambda: s.set_texture("color", 0, tex[:512]),                   # not a whole layer
    ]
    for k, call in enumerate(refused):
        with pytest.raises(frt.FrtError):
            call()
        assert snapshot(s) == before, f"refused call {k} changed the scene"
    ids = np.array([0], np.uint32)
    assert L.frt_scene_set_materials(s._h, 1, ids.ctypes.data, None) == -1                   # FRT_ERR_INVALID_ARG: a null pointer with n > 0
    assert L.frt_scene_set_instance_materials(s._h, 1, None, ids.ctypes.data) == -1
    assert L.frt_scene_set_light_emission(s._h, 0, None, 1.0) == -1
    assert L.frt_scene_set_texture(s._h, 0, 0, None) == -1
    assert L.frt_scene_set_materials(None, 0, None, None) == -1
    assert snapshot(s) == before
    # the valid halves of the refused calls are accepted on their own
    s.set_materials([0], [ok]).set_instance_materials([TALL_BOX], [RED]).set_texture("color", 3, tex)


def test_unbuilt_scene_is_a_state_error(frt):
    L = frt.lib()
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.create_plane())
    b.add_material(frt.material_new([1, 1, 1, 1]))
    b.add_instance(0, 0, np.eye(4, dtype=np.float32))
    one = np.zeros(1, np.uint32)
    m = frt.material_new([1, 0, 0, 1])
    c = np.ones(3, np.float32)
    tex = gradient_texture()
    assert L.frt_scene_set_materials(b._h, 1, one.ctypes.data, C.addressof(m)) == -4          # FRT_ERR_STATE
    assert b"not built" in L.frt_last_error()
    assert L.frt_scene_set_instance_materials(b._h, 1, one.ctypes.data, one.ctypes.data) == -4
    assert L.frt_scene_set_light_emission(b._h, 0, c.ctypes.data, 1.0) == -4
    assert L.frt_scene_set_texture(b._h, 0, 0, tex.ctypes.data) == -4
    with pytest.raises(frt.FrtError):
        b.set_materials([0], [m])
    b.build()
    assert len(b.get("materials")) == 1 and b.get("materials")[0].tobytes() == bytes(frt.material_new([1, 1, 1, 1]))   # the refused edit left no trace
    b.set_materials([0], [m])
    assert b.get("materials")[0].tobytes() == bytes(m)


def test_build_still_rejects_through_the_shared_check(frt):
    def scene_with(m):
        b = frt.SceneBuilder()
        b.add_mesh(frt.geometry.create_plane())
        b.add_material(m)
        b.add_instance(0, 0, np.eye(4, dtype=np.float32))
        return b

    cases = []
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_0 = 0xFFFF0003; cases.append((m, b"base colour texture layer 3 does not exist (3 layers)"))
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_0 = 0x0007FFFF; cases.append((m, b"normal texture layer 7 does not exist"))
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_1 = 0xFFFF0003; cases.append((m, b"occlusion texture layer 3 does not exist"))
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_1 = 0x0003FFFF; cases.append((m, b"emissive texture layer 3 does not exist"))
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_2 = 0xFFFF0009; cases.append((m, b"metallic-roughness texture layer 9 does not exist"))
    m = frt.material_new([1, 1, 1, 1]); m.light_index = 0; cases.append((m, b"material 0: light_index 0 does not exist (0 lights)"))
    for m, msg in cases:
        b = scene_with(m)
        with pytest.raises(frt.FrtError):
            b.build()
        assert msg in frt.lib().frt_last_error(), frt.lib().frt_last_error()
    m = frt.material_new([1, 1, 1, 1]); m.tex_info_0 = 0x00020002; m.tex_info_1 = 0x00020002; m.tex_info_2 = 0xFFFF0002
    scene_with(m).build()                                               # the last existing layer of each array is accepted
