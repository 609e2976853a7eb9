"""Scenes as the list of builder calls that made them, for the tests of removing materials, meshes, lights and texture layers.
Editing the list the way the library edits its scene (drop the calls that made what leaves, renumber the ids the surviving calls name) and building it
from scratch gives the reference every edited scene or replica is compared with."""
import copy
import numpy as np

BUILDER_LAYERS = 3      # colour and data layers every SceneBuilder starts with
NONE = 0xFFFF


def solid_layer(rgba):
    t = np.empty((1024, 1024, 4), np.uint8)
    t[:] = np.asarray(rgba, np.uint8)
    return t


def stripes_layer(period, a, b):
    t = np.empty((1024, 1024, 4), np.uint8)
    on = ((np.arange(1024) // period) % 2 == 0)
    t[:] = np.where(on[None, :, None], np.asarray(a, np.uint8), np.asarray(b, np.uint8))
    return t


class Calls:
    """kinds: mesh (geo), material (mat), ctex / dtex (px), light (rec), inst (mesh, mat, m), quad / sphere (mesh, m, color, intensity)."""

    def __init__(self, calls):
        self.calls = [copy.copy(c) for c in calls]

    @staticmethod
    def of_list(lst):
        """A SceneList of tests/_instance_lists.py as calls: its meshes, its materials, its entries."""
        return Calls([{"kind": "mesh", "geo": g} for g in lst.meshes] + [{"kind": "material", "mat": m} for m in lst.materials] + [copy.copy(e) for e in lst.entries])

    def plus(self, *calls):
        return Calls(self.calls + list(calls))

    @property
    def meshes(self):
        return [c["geo"] for c in self.calls if c["kind"] == "mesh"]

    def build(self, frt):
        b = frt.SceneBuilder()
        for c in self.calls:
            k = c["kind"]
            if k == "mesh":
                b.add_mesh(c["geo"])
            elif k == "material":
                b.add_material(c["mat"])
            elif k == "ctex":
                b.add_color_texture(c["px"])
            elif k == "dtex":
                b.add_data_texture(c["px"])
            elif k == "light":
                b.add_light(c["rec"])
            elif k == "quad":
                b.register_quad_light(c["mesh"], c["m"], c["color"], c["intensity"])
            elif k == "sphere":
                b.register_sphere_light(c["mesh"], c["m"], c["color"], c["intensity"])
            else:
                b.add_instance(c["mesh"], c["mat"], c["m"])
        return b.build()

    def _made_by(self, kinds):
        """Index of the call that made id 0, 1, ... of a pool."""
        return [k for k, c in enumerate(self.calls) if c["kind"] in kinds]

    def _without(self, gone_calls, mesh_map=None, mat_map=None, light_map=None, color_layer=None, data_layer=None):
        out = []
        for k, c in enumerate(self.calls):
            if k in gone_calls:
                continue
            c = copy.copy(c)
            if mesh_map is not None and "mesh" in c:
                c["mesh"] = mesh_map[c["mesh"]]
            if mat_map is not None and c["kind"] == "inst":
                c["mat"] = mat_map[c["mat"]]
            if c["kind"] == "material" and (light_map is not None or color_layer is not None or data_layer is not None):
                m = type(c["mat"]).from_buffer_copy(bytes(c["mat"]))
                if light_map is not None and m.light_index >= 0:
                    m.light_index = light_map[m.light_index]
                down = lambda s, layer: s - 1 if layer is not None and s != NONE and s > layer else s
                m.tex_info_0 = down(m.tex_info_0 & 0xFFFF, color_layer) | (down(m.tex_info_0 >> 16, data_layer) << 16)
                m.tex_info_1 = down(m.tex_info_1 & 0xFFFF, data_layer) | (down(m.tex_info_1 >> 16, color_layer) << 16)
                m.tex_info_2 = down(m.tex_info_2 & 0xFFFF, data_layer) | (m.tex_info_2 & 0xFFFF0000)
                c["mat"] = m
            out.append(c)
        return Calls(out)

    @staticmethod
    def _map(count, gone):
        m, new = {}, 0
        for i in range(count):
            if i not in gone:
                m[i] = new
                new += 1
        return m

    def material_map(self, ids):
        made = self._made_by(("material", "quad", "sphere"))
        return self._map(len(made), {int(i) for i in np.atleast_1d(ids)})

    def without_materials(self, ids):
        made = self._made_by(("material", "quad", "sphere"))
        gone = {int(i) for i in np.atleast_1d(ids)}
        assert all(self.calls[made[i]]["kind"] == "material" for i in gone)
        return self._without({made[i] for i in gone}, mat_map=self._map(len(made), gone))

    def without_meshes(self, ids):
        made = self._made_by(("mesh",))
        gone = {int(i) for i in np.atleast_1d(ids)}
        return self._without({made[i] for i in gone}, mesh_map=self._map(len(made), gone))

    def without_lights(self, ids):
        lights, mats = self._made_by(("light", "quad", "sphere")), self._made_by(("material", "quad", "sphere"))
        gone = {int(i) for i in np.atleast_1d(ids)}
        gone_calls = {lights[i] for i in gone}
        gone_mats = {j for j, k in enumerate(mats) if k in gone_calls}      # the materials the removed register_* calls made
        return self._without(gone_calls, mat_map=self._map(len(mats), gone_mats), light_map=self._map(len(lights), gone))

    def without_texture(self, kind, layer):
        made = self._made_by(("ctex" if kind == 0 else "dtex",))
        return self._without({made[layer - BUILDER_LAYERS]}, color_layer=layer if kind == 0 else None, data_layer=layer if kind == 1 else None)

    def without_instances(self, ids):
        made = self._made_by(("inst", "quad", "sphere"))
        gone = {int(i) for i in np.atleast_1d(ids)}
        assert all(self.calls[made[i]]["kind"] == "inst" for i in gone)
        return self._without({made[i] for i in gone})


def point_light(frt, pos, radius, emission):
    """A sphere light record as SceneBuilder::add_sphere_light makes it (no instance, no link)."""
    l = frt.Light()
    l.position[:] = pos
    l.type_ = 1
    l.area = float(np.float32(4.0) * np.float32(np.pi) * np.float32(radius) * np.float32(radius))
    l.v[0] = radius
    l.emission[:] = emission
    return l


def textured(frt, base, color=NONE, normal=NONE, occlusion=NONE, emissive=NONE, mr=NONE, light_index=-1):
    m = frt.material_new(base)
    m.tex_info_0 = color | (normal << 16)
    m.tex_info_1 = occlusion | (emissive << 16)
    m.tex_info_2 = mr | (m.tex_info_2 & 0xFFFF0000)
    m.light_index = light_index
    return m


def rich(frt):
    """cornell_list with what the removals need around it: unused materials in front of, between and behind the used ones' ids, an unused mesh, two
    add_light lights (one named by a material), two layers of each kind (the second named by a material)."""
    from _instance_lists import cornell_list, trs
    base = Calls.of_list(cornell_list(frt))
    first = [c for c in base.calls if c["kind"] in ("mesh", "material")]
    rest = [c for c in base.calls if c["kind"] not in ("mesh", "material")]
    extra = [{"kind": "ctex", "px": solid_layer((200, 40, 40, 255))}, {"kind": "ctex", "px": solid_layer((40, 200, 40, 255))},
             {"kind": "dtex", "px": solid_layer((128, 128, 255, 255))}, {"kind": "dtex", "px": solid_layer((255, 200, 60, 255))},
             {"kind": "light", "rec": point_light(frt, (0.5, 0.5, 0.5), 0.05, (1.0, 0.5, 0.2, 3.0))}, {"kind": "light", "rec": point_light(frt, (-0.5, 0.2, 0.4), 0.04, (0.2, 0.5, 1.0, 2.0))}]
    mats = [{"kind": "material", "mat": frt.material_new([0.1, 0.2, 0.3, 1.0])},                                       # 6: unused
            {"kind": "material", "mat": textured(frt, [0.9, 0.9, 0.9, 1.0], color=4, mr=4, light_index=1)},           # 7: names colour 4, data 4 and light 1
            {"kind": "material", "mat": frt.material_new([0.3, 0.2, 0.1, 1.0])}]                                       # 8: unused
    return Calls(first + mats + extra + rest).plus({"kind": "inst", "mesh": 1, "mat": 7, "m": trs(frt, (0.45, -0.7, 0.35), 0.4, 0.2)})
