"""src/scene/loader.rs:9-181 load_gltf over frt_model_* (parsing, PNG decode and the Lanczos3 resize happen in libfrt.so)."""
import ctypes as C
import numpy as np
from ._lib import lib, check, Material, FrtError
from .geometry import Geometry


class Model:
    """The (geometries, materials, images, material_indices) tuple load_gltf returns, held by the library."""

    def __init__(self, path):
        self._destroy = lib().frt_model_destroy
        self._h = lib().frt_model_load(str(path).encode())
        if not self._h:
            raise FrtError(lib().frt_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def counts(self):
        c = (C.c_uint32 * 4)()
        check(lib().frt_model_counts(self._h, c))
        return dict(zip(("geometries", "materials", "images", "warnings"), list(c)))

    def geometry(self, i):
        nv, ni, mi = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().frt_model_geometry_counts(self._h, i, C.byref(nv), C.byref(ni), C.byref(mi)))
        pos = np.zeros((nv.value, 4), np.float32); att = np.zeros((nv.value, 8), np.float32); idx = np.zeros(ni.value, np.uint32)
        check(lib().frt_model_geometry_get(self._h, i, pos.ctypes.data, att.ctypes.data, idx.ctypes.data))
        return Geometry(pos, att, idx), mi.value

    def material(self, i):
        m = Material()
        check(lib().frt_model_material_get(self._h, i, C.byref(m)))
        return m

    def set_material(self, i, m):
        check(lib().frt_model_material_set(self._h, i, C.byref(m)))

    def image(self, i):
        out = np.zeros((1024, 1024, 4), np.uint8)
        check(lib().frt_model_image_get(self._h, i, out.ctypes.data))
        return out

    def warnings(self):
        return [lib().frt_model_warning(self._h, i).decode() for i in range(self.counts()["warnings"])]

    # ---- the rig of a glTF document (include/frt.h: frt_model_rig_counts and the calls after it; DESIGN.md section 11, "Animation")
    def rig_counts(self):
        c = (C.c_uint32 * 3)()
        check(lib().frt_model_rig_counts(self._h, C.byref(c)))
        return dict(zip(("nodes", "skins", "animations"), list(c)))

    def _geometry_rig(self, geo):
        c = (C.c_uint32 * 4)()
        check(lib().frt_model_geometry_rig(self._h, int(geo), C.byref(c)))
        return [None if x == 0xFFFFFFFF else int(x) for x in c]

    def skin(self, geo):
        """(joints [n, 4] uint16, weights [n, 4] float32, skin index or None) of geometry `geo` in its vertex order, or None without JOINTS_0 / WEIGHTS_0."""
        has, skin, _, _ = self._geometry_rig(geo)
        if not has:
            return None
        n = len(self.geometry(geo)[0].positions)
        j, w = np.zeros((n, 4), np.uint16), np.zeros((n, 4), np.float32)
        check(lib().frt_model_geometry_skin_get(self._h, int(geo), j.ctypes.data, w.ctypes.data))
        return j, w, skin

    def morph_targets(self, geo):
        """(deltas [T, n, 3] float32, default weights [T]) of geometry `geo`, or None when its primitive has no targets."""
        t = self._geometry_rig(geo)[2]
        if not t:
            return None
        n = len(self.geometry(geo)[0].positions)
        d, w = np.zeros((t, n, 3), np.float32), np.zeros(t, np.float32)
        check(lib().frt_model_geometry_targets_get(self._h, int(geo), d.ctypes.data, w.ctypes.data))
        return d, w

    def nodes(self):
        """The node hierarchy, parents first: parents [N] (-1: a root), translations [N, 3], rotations [N, 4] (x, y, z, w), scales [N, 3], has_matrix [N],
        matrices [N, 16] (column-major) and document_index [N], the document's index of each stored node."""
        n = self.rig_counts()["nodes"]
        par, trs, has, mats, doc = np.zeros(n, np.int32), np.zeros((n, 10), np.float32), np.zeros(n, np.uint8), np.zeros((n, 16), np.float32), np.zeros(n, np.uint32)
        check(lib().frt_model_nodes_get(self._h, par.ctypes.data, trs.ctypes.data, has.ctypes.data, mats.ctypes.data, doc.ctypes.data))
        return {"parents": par, "translations": trs[:, 0:3].copy(), "rotations": trs[:, 3:7].copy(), "scales": trs[:, 7:10].copy(), "has_matrix": has.astype(bool),
                "matrices": mats, "document_index": doc}

    def skin_joints(self, skin):
        """(joint nodes [J] as stored node indices, inverse bind matrices [J, 16]) of skin `skin`."""
        nj = C.c_uint32()
        check(lib().frt_model_skin_get(self._h, int(skin), C.byref(nj), None, None))
        j, ib = np.zeros(nj.value, np.uint32), np.zeros((nj.value, 16), np.float32)
        check(lib().frt_model_skin_get(self._h, int(skin), None, j.ctypes.data, ib.ctypes.data))
        return j, ib

    def animations(self):
        """[(name, channels)], a channel a dict as frt.Rig takes it: node (stored index), path, interpolation, times [K], values [K, width] or
        [K, 3, width] (CUBICSPLINE)."""
        from ._lib import RIG_PATHS, RIG_INTERPOLATIONS
        paths, interps = {v: k for k, v in RIG_PATHS.items()}, {v: k for k, v in RIG_INTERPOLATIONS.items()}
        out = []
        for a in range(self.rig_counts()["animations"]):
            name, nch = C.c_char_p(), C.c_uint32()
            check(lib().frt_model_animation_info(self._h, a, C.byref(name), C.byref(nch)))
            channels = []
            for k in range(nch.value):
                c = (C.c_uint32 * 5)()
                check(lib().frt_model_channel_info(self._h, a, k, C.byref(c)))
                times, values = np.zeros(c[3], np.float32), np.zeros(c[4], np.float32)
                check(lib().frt_model_channel_get(self._h, a, k, times.ctypes.data, values.ctypes.data))
                values = values.reshape(c[3], 3, -1) if c[2] == 2 else values.reshape(c[3], -1)
                channels.append({"node": int(c[0]), "path": paths[c[1]], "interpolation": interps[c[2]], "times": times, "values": values})
            out.append((name.value.decode(), channels))
        return out

    def rig(self, skin=0):
        """frt.Rig of skin `skin` (None: a morph-only rig): every node, the skin's joints, the targets under it, one clip per animation."""
        from .animation import Rig
        return Rig.from_model(self, skin)

    # ---- node animation (include/frt.h: frt_model_geometry_nodes, frt_rig_from_model_nodes; DESIGN.md section 11, "Node animation")
    def geometry_nodes(self, geo):
        """The stored indices, ascending, of the nodes that carry the mesh of geometry `geo` (uint32 [k]; an OBJ model: none)."""
        n = C.c_uint32()
        check(lib().frt_model_geometry_nodes(self._h, int(geo), 0, None, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        check(lib().frt_model_geometry_nodes(self._h, int(geo), out.size, out.ctypes.data, C.byref(n)))
        return out

    def node_rig(self):
        """frt.Rig of every node, without joints and targets, one clip per animation (weights channels left out): what bind_rig_instances and
        animate_instances take for a document in which nothing is skinned."""
        from .animation import Rig
        rig = Rig.__new__(Rig)
        rig._adopt(lib().frt_rig_from_model_nodes(self._h), "frt_rig_from_model_nodes")
        rig._parents = self.nodes()["parents"]
        return rig


def bind_character(target, model, mesh_ids, skin_mode="linear"):
    """Bind what `model` holds for each of its geometries to the mesh it became: set_mesh_morph_targets for a geometry with targets, set_mesh_skin (with
    its skin's joint count) for one with skin attributes. `target`: a built scene, a Renderer or a MultiRenderer; mesh_ids[g]: the mesh id of geometry g
    (what add_gltf_meshes / add_meshes returned); skin_mode: set_mesh_skin's `mode` for every skin bound here ("linear" or "dual_quaternion"). Returns
    the mesh ids that got a binding."""
    bound = []
    for g, mesh in enumerate(mesh_ids):
        targets, skin = model.morph_targets(g), model.skin(g)
        if targets is not None:
            target.set_mesh_morph_targets(int(mesh), targets[0])
        if skin is not None and skin[2] is not None:
            target.set_mesh_skin(int(mesh), skin[0], skin[1], num_joints=len(model.skin_joints(skin[2])[0]), mode=skin_mode)
        if targets is not None or (skin is not None and skin[2] is not None):
            bound.append(int(mesh))
    return bound


def load_gltf(path):
    """.gltf / .glb (and .obj, an extension). Raises FrtError with the loader's message on failure."""
    return Model(path)
