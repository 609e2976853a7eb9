"""New meshes, materials, texture layers and lights for a running renderer (include/frt.h: frt_renderer_add_meshes and the calls after it; DESIGN.md
section 15). The specification is the host builder: after any sequence of the new calls, mixed with the older edits, the replica holds what a scene built
from scratch with the same sequence of builder calls holds. Every comparison is bit equality: of the replica's records with that scene's, of every
buffer of the frames with a renderer over it and, where cheap, with the brute-force oracle over it."""
import ctypes as C
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_instance_add_remove_gpu import CONFIGS, check_replica, check_frames, renderer
from _instance_lists import SceneList, cornell_list, one_triangle, trs

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = -1, -4
PLANE, CUBE, SPHERE = 0, 1, 2      # meshes of cornell_list (4 is its one-triangle mesh)
POOLS = ("attributes", "indices", "mesh_infos")
EVERY = ("materials", "lights", "instances_dev", "shade_tris", "tri_slots", "quad_nodes") + POOLS + ("normals",)


def encoded(frt, n):
    out = np.zeros(2, np.float32)
    frt.lib().frt_encode_octahedral_normal(np.asarray(n, np.float32).ctypes.data, out.ctypes.data)
    return out


def pyramid(frt, h=0.6):
    """5 vertices, 4 triangles (the sides): odd vertex and index counts, so whatever follows it in the pools starts at an unaligned base."""
    pos = np.array([[-0.5, 0.0, -0.5, 1.0], [0.5, 0.0, -0.5, 1.0], [0.5, 0.0, 0.5, 1.0], [-0.5, 0.0, 0.5, 1.0], [0.0, h, 0.0, 1.0]], np.float32)
    att = np.zeros((5, 8), np.float32)
    for k, n in enumerate(([-1.0, 0.4, -1.0], [1.0, 0.4, -1.0], [1.0, 0.4, 1.0], [-1.0, 0.4, 1.0], [0.0, 1.0, 0.0])):
        att[k, 0:2] = encoded(frt, np.asarray(n) / np.linalg.norm(n))
        att[k, 2:4] = [0.2 * k, 1.0 - 0.2 * k]
        att[k, 4:8] = [1.0, 0.0, 0.0, 1.0]
    return frt.geometry.Geometry(pos, att, np.array([0, 4, 1, 1, 4, 2, 2, 4, 3, 3, 4, 0], np.uint32))


def new_meshes(frt):
    return [one_triangle(frt, 0.05), frt.geometry.create_sphere(1), pyramid(frt)]


def new_materials(frt):
    a, b = frt.material_new([0.2, 0.5, 0.9, 1.0]), frt.material_new([0.9, 0.7, 0.1, 1.0])
    b.roughness, b.metallic = 0.15, 1.0
    return [a, b]


def new_transforms(frt):
    return np.stack([trs(frt, (-0.45, 0.3, 0.4), 0.5, 0.4), trs(frt, (0.0, 0.0, 1.0), 0.4, 0.3), trs(frt, (0.45, -0.99, 0.55), 0.5, -0.3)])


def host_normals(frt, meshes):
    """The host's decoded normal of every vertex of `meshes`, in pool order. The builder's decoded_vertex_normal is not exported, but a shading record
    holds what it gives for a triangle's three corners (object space: the records are not transformed). So: a scratch scene over the same vertices with
    one triangle (v, v + 1, v + 2), indices modulo the vertex count, per vertex v (a mesh may hold vertices that none of its own triangles names), one
    instance of each mesh; corner 0 of triangle v is vertex v."""
    probes = []
    for g in meshes:
        n = len(np.asarray(g.positions))
        v = np.arange(n, dtype=np.uint32)
        probes.append(type(g)(g.positions, g.attributes, np.stack([v, (v + 1) % n, (v + 2) % n], axis=1).reshape(-1).astype(np.uint32)))
    lst = SceneList(probes, [frt.material_new([1, 1, 1, 1])], [{"kind": "inst", "mesh": k, "mat": 0, "m": np.eye(4, dtype=np.float32).reshape(16)} for k in range(len(meshes))])
    s = lst.build(frt)
    assert s.counts()["tris"] == s.counts()["attributes"]      # triangle id = vertex number in pool order
    out = np.zeros((s.counts()["attributes"], 4), np.float32)
    out[:, 0:3] = s.get("shade_tris")[:, 0:3]
    return out


def check_pools(frt, r, fresh, meshes, what):
    for w in POOLS:
        got, ref = r.read_scene(w), fresh.get(w)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}: {w} differs from the scratch build"
    pc, fc = r.pool_counts(), fresh.counts()
    assert (pc["meshes"], pc["vertices"], pc["indices"]) == (fc["meshes"], fc["attributes"], fc["indices"]), what
    assert r.read_scene("normals").tobytes() == host_normals(frt, meshes).tobytes(), f"{what}: the device's decoded normals are not the host's"


# ---------------------------------------------------------------------------------------------------------------- 1. meshes
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("quality", ["morton", "sah"])
def test_meshes(gpu, orc, quality, cfg):
    frt = gpu
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), cfg)
    assert r.add_meshes(new_meshes(frt)) == 5 and r.add_materials(new_materials(frt)) == 8
    assert r.add_instances([5, 6, 7], [8, 9, 8], new_transforms(frt), quality=quality) == 9
    after = SceneList(lst.meshes + new_meshes(frt), lst.materials, lst.entries)
    # the scratch build: the Cornell list's calls (its two registered lights make materials 6 and 7), then the new materials, then the instances
    fresh = scratch(frt, after, materials=new_materials(frt), instances=([5, 6, 7], [8, 9, 8], new_transforms(frt)))
    check_replica(frt, r, fresh, f"meshes, {quality}", origin={"morton": 1, "sah": 2}[quality])
    check_pools(frt, r, fresh, after.meshes, f"meshes, {quality}")
    check_frames(frt, orc, r, after, fresh, cfg, f"meshes, {quality}, {cfg}")


def scratch(frt, lst, materials=(), textures=(), lights=(), registered=(), instances=None, build=True):
    """SceneList.build's builder calls, then: materials, (kind, pixels) layers, light records, (kind, mesh, matrix, colour, intensity) registered lights
    and (mesh ids, material ids, matrices) instances, in the order the tests below make the same calls on a renderer."""
    b = frt.SceneBuilder()
    for g in lst.meshes:
        b.add_mesh(g)
    for m in lst.materials:
        b.add_material(m)
    for e in lst.entries:
        if e["kind"] == "quad":
            b.register_quad_light(e["mesh"], e["m"], e["color"], e["intensity"])
        elif e["kind"] == "sphere":
            b.register_sphere_light(e["mesh"], e["m"], e["color"], e["intensity"])
        else:
            b.add_instance(e["mesh"], e["mat"], e["m"])
    for kind, t in textures:
        (b.add_color_texture if kind == 0 else b.add_data_texture)(t)
    for m in materials:
        b.add_material(m)
    for l in lights:
        b.add_light(l)
    for kind, mesh, m, color, intensity in registered:
        (b.register_quad_light if kind == 0 else b.register_sphere_light)(mesh, m, color, intensity)
    if instances is not None:
        for me, ma, m in zip(*instances):
            b.add_instance(int(me), int(ma), m)
    return b.build() if build else b


# ---------------------------------------------------------------------------------------------------------------- 2. one at a time
def test_one_mesh_at_a_time(gpu, orc):
    frt = gpu
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "one stream")
    added = [one_triangle(frt, 0.01 * k) if k % 2 else pyramid(frt, 0.3 + 0.05 * k) for k in range(9)]
    for k, g in enumerate(added):
        assert r.add_meshes(g) == 5 + k
        assert r.pool_counts()["meshes"] == 6 + k
    # capacities at least double: 5 meshes -> 10 -> 20 holds the 14, and the vertices and indices of nine tiny meshes fit the first doubling
    assert 1 <= r.pool_counts()["growths"] <= 4
    me, ma, m = [5, 9, 13], [0, 1, 2], new_transforms(frt)
    assert r.add_instances(me, ma, m) == 9
    after = SceneList(lst.meshes + added, lst.materials, lst.entries)
    fresh = scratch(frt, after, instances=(me, ma, m))
    check_replica(frt, r, fresh, "nine meshes")
    check_pools(frt, r, fresh, after.meshes, "nine meshes")      # (what was there before each growth included)
    check_frames(frt, orc, r, after, fresh, "one stream", "nine meshes", frames=2, oracle=False)


# ---------------------------------------------------------------------------------------------------------------- 3. textures
def patterns():
    y, x = np.mgrid[0:1024, 0:1024]
    color = np.stack([(x * 7 + y * 3) % 256, (x ^ y) % 256, (x // 4 + y // 2) % 256, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    data = np.stack([(x + y) % 256, 255 - (x // 3) % 256, 128 + (y % 128), np.full_like(x, 255)], axis=-1).astype(np.uint8)
    return color, data


def test_textures(gpu):
    frt = gpu
    flags, W, H = CONFIGS["one stream"]
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "one stream")
    color, data = patterns()
    assert r.add_texture("color", color) == 3 and r.add_texture("data", data) == 3
    mat = frt.material_new([0.9, 0.9, 0.9, 1.0])
    mat.tex_info_0 = 3 | (3 << 16); mat.tex_info_1 = 3 | (0xFFFF << 16); mat.tex_info_2 = 3 | (0xFFFF << 16)      # base colour, normal, occlusion and metallic-roughness
    assert r.add_materials(mat) == 8
    m = plane_facing_camera(frt)
    assert r.add_instances(PLANE, 8, m) == 9
    textures = [(0, color), (1, data)]
    fresh = scratch(frt, lst, materials=[mat], textures=textures, instances=([PLANE], [8], [m]))
    check_replica(frt, r, fresh, "textures")
    assert r.pool_counts()["color_layers"] == 4 and r.pool_counts()["data_layers"] == 4
    check_frames(frt, None, r, lst, fresh, "one stream", "textures", oracle=False)      # (galbedo and gnormal among every buffer of every frame)
    # ... and the new layers take set_texture
    for kind, t in ((0, color[::-1].copy()), (1, data[:, ::-1].copy())):
        r.set_texture(kind, 3, t); fresh.set_texture(kind, 3, t)
    check_frames(frt, None, r, lst, fresh, "one stream", "textures, after set_texture", frames=2, oracle=False)


def plane_facing_camera(frt):
    from frt.scenes import _T, _S, _RX, _mul
    return np.asarray(_mul(_T(0.0, 0.0, 0.9), _RX(np.pi / 2), _S(0.9)), np.float32).reshape(16)


# ---------------------------------------------------------------------------------------------------------------- 4. lights
def light_records(frt):
    quad, sphere = frt.Light(), frt.Light()
    quad.position[:] = [-0.6, 0.5, 0.2]; quad.u[:] = [0.1, 0.0, 0.0]; quad.v[:] = [0.0, 0.0, -0.15]; quad.type_ = 0
    quad.area = float(np.float32(0.1 * 0.15 * 4.0)); quad.emission[:] = [1.0, 0.5, 0.2, 6.0]
    sphere.position[:] = [0.5, 0.2, 0.5]; sphere.v[0] = 0.07; sphere.type_ = 1
    sphere.area = float(np.float32(4.0 * np.pi * 0.07 * 0.07)); sphere.emission[:] = [0.3, 1.0, 0.4, 8.0]
    return [quad, sphere]


def registered_lights(frt):
    from frt.scenes import _T, _S, _RX, _mul
    q = np.asarray(_mul(_T(-0.4, 0.98, 0.4), _RX(np.pi), _S(0.3)), np.float32).reshape(16)
    s = np.asarray(_mul(_T(-0.5, -0.6, 0.5), _S(0.12)), np.float32).reshape(16)
    return [(0, PLANE, q, (1.0, 0.8, 0.6), 7.0), (1, SPHERE, s, (0.2, 0.9, 0.3), 9.0)]


def apply_lights(frt, x, quality="sah"):
    """Case 4's calls on a Renderer or a MultiRenderer: two light records, then a registered quad and a registered sphere light."""
    assert x.add_lights(light_records(frt)) == 2
    for kind, mesh, m, color, intensity in registered_lights(frt):
        got = (x.register_quad_light if kind == 0 else x.register_sphere_light)(mesh, m, color, intensity, quality=quality)
        assert got == 4 + kind


@pytest.mark.parametrize("cfg,quality", [("one stream", "sah"), ("pipeline", "morton")])
def test_lights(gpu, orc, cfg, quality):
    frt = gpu
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), cfg)
    assert r.add_lights(light_records(frt)) == 2
    fresh = scratch(frt, lst, lights=light_records(frt))
    assert fresh.num_lights == 4
    check_replica(frt, r, fresh, "add_lights", origin=0)      # (no triangle was added: the tree is still the host build's)
    check_frames(frt, orc, r, lst, fresh, cfg, f"add_lights, {cfg}", frames=2)      # (the cameras carry the new num_lights)
    for kind, mesh, m, color, intensity in registered_lights(frt):
        assert (r.register_quad_light if kind == 0 else r.register_sphere_light)(mesh, m, color, intensity, quality=quality) == 4 + kind
    fresh = scratch(frt, lst, lights=light_records(frt), registered=registered_lights(frt))
    assert r.scene_counts() == {"tris": fresh.counts()["tris"], "instances": 11, "materials": 10, "lights": 6}
    check_replica(frt, r, fresh, "register_*_light", origin={"morton": 1, "sah": 2}[quality])
    check_frames(frt, orc, r, lst, fresh, cfg, f"register_*_light, {cfg}", oracle=cfg == "one stream")      # (brute force over the second sphere's 1280 triangles: once)
    # the new instances behave like any registered light's
    moved = trs(frt, (0.3, 0.9, 0.2), 0.25, 0.5)
    for x in (r, fresh):
        x.set_instance_transforms([9], [moved])
        x.set_light_emission(5, (0.9, 0.1, 0.1), 4.0)
    for w in ("lights", "materials", "instances_dev", "shade_tris"):
        assert r.read_scene(w).tobytes() == fresh.get(w).tobytes(), f"after the move and the emission edit: {w}"
    nine, zero = np.array([9], np.uint32), np.array([0], np.uint32)
    assert frt.lib().frt_renderer_remove_instances(r._h, 1, nine.ctypes.data, 1) == ERR_INVALID_ARG
    assert frt.lib().frt_renderer_set_instance_materials(r._h, 1, nine.ctypes.data, zero.ctypes.data) == ERR_INVALID_ARG
    check_frames(frt, orc, r, lst, fresh, cfg, "after the move and the emission edit", frames=2, oracle=False)


# ---------------------------------------------------------------------------------------------------------------- 5. later edits on new things
def test_later_edits_on_new_things(gpu, orc):
    frt = gpu
    flags, W, H = CONFIGS["one stream"]
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "one stream")
    r.add_meshes(new_meshes(frt)); r.add_materials(new_materials(frt))
    r.add_instances([5, 6, 7], [8, 9, 8], new_transforms(frt))
    after = SceneList(lst.meshes + new_meshes(frt), lst.materials, lst.entries)
    host = scratch(frt, after, materials=new_materials(frt), instances=([5, 6, 7], [8, 9, 8], new_transforms(frt)))
    ico = frt.geometry.create_sphere(1)
    pos = np.array(ico.positions, np.float32); pos[:, 1] *= 1.3
    att = np.array(ico.attributes, np.float32); att[:, 0:2] = att[::-1, 0:2]; att[:, 2:4] = 0.5
    glossy = frt.material_new([0.1, 0.9, 0.4, 1.0]); glossy.roughness = 0.05
    for x in (r, host):
        x.set_mesh_vertices(6, pos, att)
        x.set_materials([9], [glossy])
    r.rebuild_tree("sah")
    check_replica(frt, r, host, "edits on the new mesh and the new material")
    deformed = list(after.meshes); deformed[6] = frt.geometry.Geometry(pos, att, ico.indices)
    check_pools(frt, r, host, deformed, "edits on the new mesh and the new material")
    cam = frt.CameraController().build_uniform(W / H, 0, 2)
    hit = r.pick(cam, [[W // 2, H // 2]])      # the icosphere sits between the camera and the room's centre
    assert hit["instance"][0] == 10 and hit["material"][0] == 9 and hit["primitive"][0] < 80 and hit["tri"][0] == host.get("instances")[10][2] + hit["primitive"][0]
    want = host.trace_closest([[0.0, 0.0, 2.9]], [[0.0, 0.0, -1.0]])
    got = r.trace_closest([[0.0, 0.0, 2.9]], [[0.0, 0.0, -1.0]])
    assert all(got[k].tobytes() == want[k].tobytes() for k in got) and got["instance"][0] == 10
    check_frames(frt, orc, r, SceneList(deformed, lst.materials, lst.entries), host, "one stream", "edits on new things", frames=2)


# ---------------------------------------------------------------------------------------------------------------- 6. history
def test_history_is_kept(gpu):
    frt = gpu
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "pipeline", frames=4)
    keep = lambda: [r.read_buffer(frt.BUF_ACCUM, 0).tobytes(), r.read_buffer(frt.BUF_ACCUM, 1).tobytes(), r.read_buffer(frt.BUF_RESERVOIR, 0).tobytes(), r.read_buffer(frt.BUF_RESERVOIR, 1).tobytes()]
    color, data = patterns()
    q, s = registered_lights(frt)
    calls = [lambda: r.add_meshes(new_meshes(frt)), lambda: r.add_materials(new_materials(frt)), lambda: r.add_texture(0, color), lambda: r.add_texture(1, data),
             lambda: r.add_lights(light_records(frt)), lambda: r.register_quad_light(*q[1:]), lambda: r.register_sphere_light(*s[1:])]
    for k, call in enumerate(calls):
        before, fc, dropped = keep(), r.frame_count, r.stats()["discarded_speculations"]
        call()
        assert r.frame_count == fc and keep() == before, f"call {k} touched the history"
        assert r.stats()["discarded_speculations"] == dropped + 1, f"call {k}: the frame that ran ahead was not dropped"
        for f in (fc, fc + 1):      # the sequence goes on; the second frame's camera is the one the first predicted, so the next frame runs ahead again
            r.render(frt.CameraController().build_uniform(W / H, f, r.scene_counts()["lights"]))
        assert r.frame_count == fc + 2


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing(gpu):
    frt = gpu
    L = frt.lib()
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "pipeline")
    r.add_meshes(one_triangle(frt))      # (the pools have their capacities and the decoded normals exist: a refusal must not move them either)
    state = lambda: ({w: r.read_scene(w).tobytes() for w in EVERY}, r.pool_counts(), r.scene_counts(), r.tree_stats(), r.frame_count)
    before = state()
    from frt._lib import MeshData
    tri = one_triangle(frt)
    pos, att, idx = np.ascontiguousarray(tri.positions, np.float32), np.ascontiguousarray(tri.attributes, np.float32), np.ascontiguousarray(tri.indices, np.uint32)

    good = MeshData(pos.ctypes.data, att.ctypes.data, idx.ctypes.data, 3, 3)

    def add_mesh(pos=pos, att=att, idx=idx, nverts=3, nidx=3, first_ok=False):
        a = [p.ctypes.data if p is not None else None for p in (pos, att, idx)]
        recs = (MeshData * 2)(good, MeshData(a[0], a[1], a[2], nverts, nidx))      # (first_ok: a good mesh in front, of which nothing may be applied)
        return L.frt_renderer_add_meshes(r._h, 2, recs) if first_ok else L.frt_renderer_add_meshes(r._h, 1, C.byref(recs, C.sizeof(MeshData)))
    nan_pos = pos.copy(); nan_pos[1, 2] = np.nan
    inf_att = att.copy(); inf_att[2, 5] = np.inf
    refused = {"null meshes": lambda: L.frt_renderer_add_meshes(r._h, 1, None), "null positions": lambda: add_mesh(pos=None), "null attributes": lambda: add_mesh(att=None),
               "null indices": lambda: add_mesh(idx=None), "no vertices": lambda: add_mesh(nverts=0), "no indices": lambda: add_mesh(nidx=0),
               "indices not a multiple of 3": lambda: add_mesh(idx=np.array([0, 1, 2, 0], np.uint32), nidx=4), "index out of range": lambda: add_mesh(idx=np.array([0, 1, 3], np.uint32)),
               "non-finite position": lambda: add_mesh(pos=nan_pos), "non-finite attribute": lambda: add_mesh(att=inf_att),
               "the second of two meshes is bad": lambda: add_mesh(pos=nan_pos, first_ok=True)}
    no_layer = frt.material_new([1, 1, 1, 1]); no_layer.tex_info_0 = 3 | (0xFFFF << 16)      # colour layer 3 does not exist (yet)
    no_light = frt.material_new([1, 1, 1, 1]); no_light.light_index = 2
    fine = frt.material_new([1, 1, 1, 1])
    two = (frt.Material * 2)(fine, no_layer)
    refused.update({"null materials": lambda: L.frt_renderer_add_materials(r._h, 1, None), "a layer that does not exist": lambda: L.frt_renderer_add_materials(r._h, 1, C.byref(no_layer)),
                    "a light that does not exist": lambda: L.frt_renderer_add_materials(r._h, 1, C.byref(no_light)), "the second of two materials is bad": lambda: L.frt_renderer_add_materials(r._h, 2, two)})
    quad, sphere = light_records(frt)
    bad_light = frt.Light.from_buffer_copy(bytes(quad)); bad_light.u[1] = float("nan")
    flat_light = frt.Light.from_buffer_copy(bytes(sphere)); flat_light.area = 0.0
    color, _ = patterns()
    eye = np.eye(4, dtype=np.float32).reshape(16)
    flat = eye.copy(); flat[5] = 0.0
    white = np.ones(3, np.float32)
    reg = lambda mesh=0, m=eye, c=white, mode=1, f=L.frt_renderer_register_quad_light: f(r._h, mesh, m.ctypes.data if m is not None else None, c.ctypes.data if c is not None else None, 5.0, mode)
    refused.update({"null lights": lambda: L.frt_renderer_add_lights(r._h, 1, None), "non-finite light": lambda: L.frt_renderer_add_lights(r._h, 1, C.byref(bad_light)),
                    "light without area": lambda: L.frt_renderer_add_lights(r._h, 1, C.byref(flat_light)), "texture kind 2": lambda: L.frt_renderer_add_texture(r._h, 2, color.ctypes.data),
                    "null pixels": lambda: L.frt_renderer_add_texture(r._h, 0, None), "register: mesh out of range": lambda: reg(mesh=6), "register: singular matrix": lambda: reg(m=flat),
                    "register: null colour": lambda: reg(c=None), "register: unknown rebuild mode": lambda: reg(mode=2),
                    "register sphere: null matrix": lambda: reg(m=None, f=L.frt_renderer_register_sphere_light)})
    for what, call in refused.items():
        assert call() == ERR_INVALID_ARG, (what, L.frt_last_error())
        assert state() == before, f"{what}: a refused call changed the replica"
    assert L.frt_renderer_add_meshes(r._h, 0, None) == 6 and L.frt_renderer_add_materials(r._h, 0, None) == 8 and L.frt_renderer_add_lights(r._h, 0, None) == 2      # n == 0
    assert L.frt_renderer_add_meshes(None, 0, None) == ERR_INVALID_ARG
    assert state() == before
    cam = frt.CameraController().build_uniform(W / H, 2, 2)
    r.render_phases(cam, frt.PHASE_GBUFFER)      # a frame is open
    one = (MeshData * 1)(good)
    opened = {"add_meshes": lambda: L.frt_renderer_add_meshes(r._h, 1, one), "add_materials": lambda: L.frt_renderer_add_materials(r._h, 1, C.byref(fine)),
              "add_texture": lambda: L.frt_renderer_add_texture(r._h, 0, color.ctypes.data), "add_lights": lambda: L.frt_renderer_add_lights(r._h, 1, C.byref(quad)),
              "register_quad_light": reg, "register_sphere_light": lambda: reg(f=L.frt_renderer_register_sphere_light)}
    for what, call in opened.items():
        assert call() == ERR_STATE and b"frame is open" in L.frt_last_error(), what
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    after = state()
    assert after[0] == before[0] and after[1:4] == before[1:4] and after[4] == before[4] + 1


# ---------------------------------------------------------------------------------------------------------------- 8. two strips
def test_two_strips(gpu):
    frt = gpu
    flags, W, H = CONFIGS["pipeline"]
    lst = cornell_list(frt)
    one = frt.Renderer(lst.build(frt), W, H, max_depth=8, flags=flags)
    two = frt.MultiRenderer(lst.build(frt), W, H, [0, 0], max_depth=8, flags=flags)

    def frames(lo, hi, lights):
        for f in range(lo, hi):
            cam = frt.CameraController().build_uniform(W / H, f, lights)
            one.render(cam); two.render(cam)
            for b, idx in ((frt.BUF_ACCUM, 0), (frt.BUF_ACCUM, 1), (frt.BUF_DISPLAY, 0), (frt.BUF_RAW, 0), (frt.BUF_RESERVOIR, 0), (frt.BUF_RESERVOIR, 1)):
                assert one.read_buffer(b, idx).tobytes() == two.read_buffer(b, idx).tobytes(), f"frame {f}, buffer {b}[{idx}]"

    frames(0, 2, 2)
    for x in (one, two):
        assert x.add_meshes(new_meshes(frt)) == 5 and x.add_materials(new_materials(frt)) == 8
        assert x.add_instances([5, 6, 7], [8, 9, 8], new_transforms(frt)) == 9
    frames(2, 4, 2)
    for x in (one, two):
        apply_lights(frt, x)
    frames(4, 6, 6)
    color, _ = patterns()
    assert one.add_texture(0, color) == 3 and two.add_texture(0, color) == 3
    cam = frt.CameraController().build_uniform(W / H, 5, 6)
    hit, want = two.pick(cam, [[W // 2, H // 2]]), one.pick(cam, [[W // 2, H // 2]])
    assert all(hit[k].tobytes() == want[k].tobytes() for k in hit) and hit["instance"][0] == 10


# ---------------------------------------------------------------------------------------------------------------- 9. glTF
def test_gltf(gpu, tmp_path):
    frt = gpu
    from test_loader import _sphere_model
    path, _ = _sphere_model(tmp_path, frt)
    model = frt.loader.load_gltf(path)
    lst = cornell_list(frt)
    r = renderer(frt, lst.build(frt), "one stream")
    m = trs(frt, (0.1, -0.2, 0.6), 0.5, 0.7)
    mesh_ids, mat_ids, first = r.add_gltf(model, m)
    b = scratch(frt, lst, build=False)
    want_mats = b.add_gltf_materials(model)
    want_meshes = b.add_gltf_meshes(model)
    b.add_gltf_instances(model, want_meshes, want_mats, m)
    fresh = b.build()
    assert list(mesh_ids) == list(want_meshes) and list(mat_ids) == list(want_mats) and first == 9
    check_replica(frt, r, fresh, "glTF")
    geos = [model.geometry(i)[0] for i in range(model.counts()["geometries"])]
    check_pools(frt, r, fresh, lst.meshes + geos, "glTF")
    pc = r.pool_counts()
    assert pc["color_layers"] + pc["data_layers"] > 6 and pc["growths"] >= 1
    check_frames(frt, None, r, lst, fresh, "one stream", "glTF", frames=2, oracle=False)
