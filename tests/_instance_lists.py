"""Scenes as plain lists, for the tests of adding and removing instances: meshes, materials and, in order, the calls that made the
instances (add_instance, register_quad_light, register_sphere_light). A list builds the scene from scratch through the public builder, and editing
the list the way the library edits its scene gives the from-scratch reference every edited scene or replica is compared with."""
import copy
import numpy as np

# every array selector of frt_scene_get that SceneBuilder.get names (selector 14, the 8-wide tree's child boxes, is read by child_boxes below)
SELECTORS = ("tris", "tri_instance", "materials", "lights", "attributes", "indices", "mesh_infos", "instances", "bvh2_nodes", "bvh2_tri_index", "quad_nodes",
             "wide8_nodes", "tri_slots8", "tri_slots", "pair_nodes", "instances_dev", "shade_tris")


def child_boxes(frt, s):
    boxes = np.zeros(s.tree_stats()["wide8_nodes"] * 48, np.float32)
    assert frt.lib().frt_scene_get(s._h, 14, boxes.ctypes.data) == 0
    return boxes


def snapshot(frt, s):
    """Everything frt_scene_get, tree_stats and bvh_stats tell about a built scene, as bytes."""
    d = {w: s.get(w).tobytes() for w in SELECTORS}
    d["wide8_child_boxes"] = child_boxes(frt, s).tobytes()
    d["tree_stats"], d["bvh_stats"], d["counts"] = s.tree_stats(), s.bvh_stats(), s.counts()
    return d


def assert_same_scene(frt, got, want, what):
    a, b = snapshot(frt, got), snapshot(frt, want)
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs from the scene built from scratch"


class SceneList:
    def __init__(self, meshes, materials, entries):
        self.meshes, self.materials, self.entries = list(meshes), list(materials), list(entries)

    def build(self, frt):
        b = frt.SceneBuilder()
        for g in self.meshes:
            b.add_mesh(g)
        for m in self.materials:
            b.add_material(m)
        for e in self.entries:
            if e["kind"] == "quad":
                b.register_quad_light(e["mesh"], e["m"], e["color"], e["intensity"])
            elif e["kind"] == "sphere":
                b.register_sphere_light(e["mesh"], e["m"], e["color"], e["intensity"])
            else:
                b.add_instance(e["mesh"], e["mat"], e["m"])
        return b.build()

    def removed(self, ids):
        gone = {int(i) for i in np.atleast_1d(ids)}
        return SceneList(self.meshes, self.materials, [copy.copy(e) for k, e in enumerate(self.entries) if k not in gone])

    def added(self, mesh_ids, mat_ids, mats):
        mats = np.asarray(mats, np.float32).reshape(-1, 16)
        new = [{"kind": "inst", "mesh": int(me), "mat": int(ma), "m": mats[k].copy()} for k, (me, ma) in enumerate(zip(np.atleast_1d(mesh_ids), np.atleast_1d(mat_ids)))]
        return SceneList(self.meshes, self.materials, [copy.copy(e) for e in self.entries] + new)

    def moved(self, k, m):
        out = SceneList(self.meshes, self.materials, [copy.copy(e) for e in self.entries])
        out.entries[k]["m"] = np.asarray(m, np.float32).reshape(16).copy()
        return out

    def with_material(self, k, mat):
        out = SceneList(self.meshes, self.materials, [copy.copy(e) for e in self.entries])
        out.entries[k]["mat"] = int(mat)
        return out

    def with_mesh(self, k, geo):
        out = SceneList(self.meshes, self.materials, [copy.copy(e) for e in self.entries])
        out.meshes[k] = geo
        return out


def one_triangle(frt, z=0.0):
    """A one-triangle mesh with its own normal, uvs and tangent at every corner (so that a wrong corner shows in the shading record)."""
    pos = np.array([[-0.5, -0.5, z, 1.0], [0.5, -0.5, z, 1.0], [0.0, 0.5, z, 1.0]], np.float32)
    att = np.zeros((3, 8), np.float32)
    for k, n in enumerate(([0.0, 0.0, 1.0], [0.1, 0.0, 0.995], [0.0, 0.1, 0.995])):
        enc = np.zeros(2, np.float32)
        frt.lib().frt_encode_octahedral_normal(np.asarray(n, np.float32).ctypes.data, enc.ctypes.data)
        att[k, 0:2] = enc
        att[k, 2:4] = [0.25 * k, 1.0 - 0.5 * k]
        att[k, 4:8] = [1.0, 0.0, 0.0, -1.0 if k == 0 else 1.0]
    return frt.geometry.Geometry(pos, att, np.arange(3, dtype=np.uint32))


def cornell_list(frt):
    """The Cornell Box of scenes.rs as a list (instance order and materials as frt.scenes.create_cornell_box makes them), with a one-triangle mesh (4) added
    that no instance uses yet."""
    from test_instance_update import cornell_meshes, QUAD_LIGHT, SPHERE_LIGHT
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    entries = []
    for k, row in enumerate(inst):
        m = row[5:21].view(np.float32).copy()
        if k == QUAD_LIGHT:
            entries.append({"kind": "quad", "mesh": int(row[0]), "m": m, "color": (1.0, 1.0, 1.0), "intensity": 10.0})
        elif k == SPHERE_LIGHT:
            entries.append({"kind": "sphere", "mesh": int(row[0]), "m": m, "color": (0.02, 0.02, 0.9), "intensity": 10.0})
        else:
            entries.append({"kind": "inst", "mesh": int(row[0]), "mat": int(row[1]), "m": m})
    materials = [frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()) for k in range(6)]
    return SceneList(cornell_meshes(frt) + [one_triangle(frt)], materials, entries)


def trs(frt, t, s=1.0, ry=0.0):
    from frt.scenes import _T, _S, _RY, _mul
    return np.asarray(_mul(_T(*t), _RY(ry), _S(s)), np.float32).reshape(16)


def odd_list(frt):
    """15 triangles: a cube and a one-triangle mesh in front of it, two materials, a quad light (a plane) above (registered, so one instance cannot be removed)."""
    g = frt.geometry
    mats = [frt.material_new([0.7, 0.3, 0.2, 1.0]), frt.material_new([0.2, 0.6, 0.8, 1.0])]
    from frt.scenes import _T, _S, _RX, _mul
    light = np.asarray(_mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.8)), np.float32).reshape(16)
    entries = [{"kind": "inst", "mesh": 0, "mat": 0, "m": trs(frt, (0.0, 0.0, -0.5), 0.8, 0.3)},
               {"kind": "quad", "mesh": 2, "m": light, "color": (1.0, 0.9, 0.8), "intensity": 6.0},
               {"kind": "inst", "mesh": 1, "mat": 1, "m": trs(frt, (0.1, 0.0, 0.6), 0.7)}]
    return SceneList([g.create_cube(), one_triangle(frt), g.create_plane()], mats, entries)


def two_instance_list(frt):
    """One mesh (a plane, 2 triangles), two instances of it, one material."""
    from frt.scenes import _T, _S, _RX, _mul
    up = lambda y, s: np.asarray(_mul(_T(0.0, y, 0.0), _RX(np.pi / 2), _S(s)), np.float32).reshape(16)
    entries = [{"kind": "inst", "mesh": 0, "mat": 0, "m": up(0.0, 1.5)}, {"kind": "inst", "mesh": 0, "mat": 0, "m": up(0.2, 0.6)}]
    return SceneList([frt.geometry.create_plane()], [frt.material_new([0.6, 0.6, 0.6, 1.0])], entries)
