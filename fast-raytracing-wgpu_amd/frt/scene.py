"""SceneBuilder mirror (src/scene/builder.rs) over frt_scene_*."""
import ctypes as C
import numpy as np
from ._lib import lib, check, Material, Light, MeshData, FrtError, DEFORM_RECOMPUTE_NORMALS


def material_new(base_color):
    """Material::new (material.rs:31-47)."""
    m = Material()
    a = np.asarray(base_color, np.float32)
    lib().frt_material_default(a.ctypes.data, C.byref(m))
    return m


def transform_args(ids, transforms_colmajor):
    """(n, ids, matrices) for the *_set_instance_transforms calls: `ids` an int or a sequence, `transforms_colmajor` one column-major
    4x4 (as frt.scenes writes them: m[4*c + r]) per id, shaped [n, 4, 4], [n, 16], [4, 4] or [16]."""
    ids = np.ascontiguousarray(np.atleast_1d(np.asarray(ids, np.int64)))
    if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise FrtError("instance ids must be a flat list of unsigned 32-bit indices")
    m = np.ascontiguousarray(transforms_colmajor, np.float32).reshape(-1, 16)
    if m.shape[0] != ids.size:
        raise FrtError(f"{ids.size} instance ids but {m.shape[0]} matrices")
    return ids.size, ids.astype(np.uint32), m


def mesh_vertex_args(mesh_id, positions, attributes):
    """(mesh id, positions, attributes or None, vertex count) for the *_set_mesh_vertices calls: `positions` [n, 4] (xyzw, as frt.geometry
    writes them), `attributes` [n, 8] (octahedral normal, uv, tangent) or None to keep the mesh's attributes."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    pos = np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 4:
        raise FrtError("positions must be shaped [n, 4]")
    att = None
    if attributes is not None:
        att = np.ascontiguousarray(attributes, np.float32).reshape(-1, 8)
        if att.shape[0] != pos.shape[0]:
            raise FrtError(f"{pos.shape[0]} positions but {att.shape[0]} attribute records")
    return int(mesh_id), pos, att, pos.shape[0]


def deform_flags(normals):
    """The flags of the *_set_mesh_vertices_ex calls for `normals`: "keep" (the attributes' normals stay) or "recompute" (every vertex normal is
    computed from the new positions: the normalised sum of the area-weighted normals of the triangles around the vertex)."""
    if normals not in ("keep", "recompute"):
        raise FrtError(f'set_mesh_vertices: normals must be "keep" or "recompute", not {normals!r}')
    return DEFORM_RECOMPUTE_NORMALS if normals == "recompute" else 0


def set_mesh_vertices_call(name, handle, mesh_id, positions, attributes, normals):
    """One host-array deformation through the entry point `name` (its _ex form when a flag is set)."""
    flags = deform_flags(normals)
    mid, pos, att, n = mesh_vertex_args(mesh_id, positions, attributes)
    a = att.ctypes.data if att is not None else None
    if flags:
        check(getattr(lib(), name + "_ex")(handle, mid, pos.ctypes.data, a, n, flags))
    else:
        check(getattr(lib(), name)(handle, mid, pos.ctypes.data, a, n))


def mesh_skin_args(mesh_id, joints, weights):
    """(mesh id, joints, weights, vertex count) for the *_set_mesh_skin calls: `joints` [n, 4] integers (converted to uint16 after a range check),
    `weights` [n, 4] float32."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    j = np.asarray(joints)
    if j.ndim != 2 or j.shape[1] != 4 or j.dtype.kind not in "iu":
        raise FrtError("set_mesh_skin: joints must be integers shaped [n, 4]")
    if j.size and (int(j.min()) < 0 or int(j.max()) > 0xFFFF):
        raise FrtError("set_mesh_skin: a joint index is an unsigned 16-bit number")
    w = np.ascontiguousarray(weights, np.float32)
    if w.ndim != 2 or w.shape[1] != 4 or w.shape[0] != j.shape[0]:
        raise FrtError(f"set_mesh_skin: weights must be shaped [{j.shape[0]}, 4], like the joints")
    return int(mesh_id), np.ascontiguousarray(j.astype(np.uint16)), w, j.shape[0]


def _num_joints(joints, num_joints):
    """The joint count a bind call states: `num_joints`, or the largest joint index + 1."""
    if num_joints is not None or joints is None:
        return int(num_joints or 0)
    j = np.asarray(joints)
    return int(j.max()) + 1 if j.size else 0


SKIN_MODES = {"linear": 0, "dual_quaternion": 1}      # include/frt.h: 0, FRT_SKIN_DUAL_QUATERNION


def set_mesh_skin_call(name, handle, mesh_id, joints, weights, njoints, mode="linear"):
    """One bind call through the entry point `name`; joints None removes the skin. `mode`: "linear" (the call `name` itself) or "dual_quaternion"
    (`name`_ex with FRT_SKIN_DUAL_QUATERNION); anything else is refused before the library is called."""
    if not isinstance(mode, str) or mode not in SKIN_MODES:
        raise FrtError(f"set_mesh_skin: mode must be 'linear' or 'dual_quaternion', not {mode!r}")
    if joints is None:
        return check(getattr(lib(), name)(handle, int(mesh_id), None, None, 0, 0))
    mid, j, w, n = mesh_skin_args(mesh_id, joints, weights)
    if SKIN_MODES[mode]:
        return check(getattr(lib(), name + "_ex")(handle, mid, j.ctypes.data, w.ctypes.data, n, int(njoints), SKIN_MODES[mode]))
    check(getattr(lib(), name)(handle, mid, j.ctypes.data, w.ctypes.data, n, int(njoints)))


def mesh_pose_args(mesh_id, joint_matrices):
    """(mesh id, [J, 16] float32 matrices, J) for the host form of the *_set_mesh_pose calls: `joint_matrices` one column-major 4x4 per joint, shaped
    [J, 16] or [J, 4, 4]."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    m = np.ascontiguousarray(joint_matrices, np.float32)
    if not (m.ndim == 2 and m.shape[1] == 16) and not (m.ndim == 3 and m.shape[1:] == (4, 4)):
        raise FrtError("set_mesh_pose: joint matrices must be shaped [J, 16] or [J, 4, 4]")
    m = m.reshape(-1, 16)
    return int(mesh_id), m, m.shape[0]


def set_mesh_pose_call(name, handle, mesh_id, joint_matrices, normals, morph_weights=None):
    """One host-array pose through the entry point `name`; with `morph_weights` the morph-and-skin call `name`_ex."""
    flags = deform_flags(normals)
    mid, m, n = mesh_pose_args(mesh_id, joint_matrices)
    if morph_weights is None:
        return check(getattr(lib(), name)(handle, mid, m.ctypes.data, n, flags))
    _, w, t = mesh_morph_weight_args(mesh_id, morph_weights)
    check(getattr(lib(), name + "_ex")(handle, mid, m.ctypes.data, n, w.ctypes.data, t, flags))


def mesh_morph_target_args(mesh_id, deltas):
    """(mesh id, deltas, vertex count, target count) for the *_set_mesh_morph_targets calls: `deltas` [T, n, 3] float32, one position delta per target
    and vertex."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    d = np.ascontiguousarray(deltas, np.float32)
    if d.ndim != 3 or d.shape[2] != 3:
        raise FrtError("set_mesh_morph_targets: deltas must be shaped [T, n, 3]")
    return int(mesh_id), d, d.shape[1], d.shape[0]


def set_mesh_morph_targets_call(name, handle, mesh_id, deltas):
    """One bind call through the entry point `name`; deltas None removes the targets."""
    if deltas is None:
        return check(getattr(lib(), name)(handle, int(mesh_id), None, 0, 0))
    mid, d, n, t = mesh_morph_target_args(mesh_id, deltas)
    check(getattr(lib(), name)(handle, mid, d.ctypes.data, n, t))


def mesh_morph_weight_args(mesh_id, weights):
    """(mesh id, [T] float32 weights, T) for the host form of the calls that take morph weights."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    w = np.ascontiguousarray(weights, np.float32)
    if w.ndim != 1:
        raise FrtError("morph weights must be shaped [T]")
    return int(mesh_id), w, w.shape[0]


def set_mesh_morph_weights_call(name, handle, mesh_id, weights, normals):
    """One host-array morph through the entry point `name`."""
    flags = deform_flags(normals)
    mid, w, t = mesh_morph_weight_args(mesh_id, weights)
    check(getattr(lib(), name)(handle, mid, w.ctypes.data, t, flags))


def pose_batch_ids(mesh_ids):
    """[n] uint32 mesh ids for the *_set_mesh_poses calls: an int or a flat sequence of unsigned 32-bit indices."""
    ids = np.atleast_1d(np.asarray(mesh_ids, np.int64))
    if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise FrtError("set_mesh_poses: mesh ids must be a flat list of unsigned 32-bit indices")
    return np.ascontiguousarray(ids.astype(np.uint32))


def set_mesh_poses_call(name, handle, mesh_ids, joint_matrices, morph_weights, normals):
    """One host-array batched pose through the entry point `name`: a palette, morph weights or both (None: not given)."""
    flags = deform_flags(normals)
    ids = pose_batch_ids(mesh_ids)
    if joint_matrices is None and morph_weights is None:
        raise FrtError("set_mesh_poses: give joint_matrices, morph_weights or both")
    m, j = (None, 0) if joint_matrices is None else mesh_pose_args(0, joint_matrices)[1:]
    w, t = (None, 0) if morph_weights is None else mesh_morph_weight_args(0, morph_weights)[1:]
    check(getattr(lib(), name)(handle, ids.size, ids.ctypes.data, m.ctypes.data if m is not None else None, j, w.ctypes.data if w is not None else None, t, flags))


def material_args(ids, materials):
    """(n, ids, [n, 16] uint32 material records) for the *_set_materials calls: `ids` an int or a sequence, `materials` one frt.Material (or a 64-byte
    row of get("materials")) per id."""
    ids = np.ascontiguousarray(np.atleast_1d(np.asarray(ids, np.int64)))
    if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise FrtError("material ids must be a flat list of unsigned 32-bit indices")
    if isinstance(materials, Material):
        materials = [materials]
    rows = [np.frombuffer(bytes(m), np.uint32) if isinstance(m, Material) else np.ascontiguousarray(m).view(np.uint32).reshape(-1) for m in materials]
    if any(r.size != 16 for r in rows):
        raise FrtError("a material is 64 bytes")
    if len(rows) != ids.size:
        raise FrtError(f"{ids.size} material ids but {len(rows)} materials")
    m = np.ascontiguousarray(np.stack(rows), np.uint32) if rows else np.zeros((0, 16), np.uint32)
    return ids.size, ids.astype(np.uint32), m


def id_pair_args(instance_ids, material_ids):
    """(n, instance ids, material ids) for the *_set_instance_materials calls."""
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(instance_ids, np.int64)))
    b = np.ascontiguousarray(np.atleast_1d(np.asarray(material_ids, np.int64)))
    if a.ndim != 1 or b.ndim != 1 or a.size != b.size:
        raise FrtError(f"{a.size} instance ids but {b.size} material ids")
    if a.size and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) > 0xFFFFFFFF):
        raise FrtError("instance and material ids must be unsigned 32-bit indices")
    return a.size, a.astype(np.uint32), b.astype(np.uint32)


def instance_add_args(mesh_ids, mat_ids, transforms_colmajor):
    """(n, mesh ids, material ids, matrices) for the *_add_instances calls: one mesh id, one material id and one column-major 4x4 per new instance
    (ints and a single matrix for one instance)."""
    n, me, ma = id_pair_args(mesh_ids, mat_ids)
    m = np.ascontiguousarray(transforms_colmajor, np.float32).reshape(-1, 16)
    if m.shape[0] != n:
        raise FrtError(f"{n} mesh ids but {m.shape[0]} matrices")
    return n, me, ma, m


def instance_id_args(ids):
    """(n, ids) for the *_remove_instances calls: `ids` an int or a sequence."""
    ids = np.ascontiguousarray(np.atleast_1d(np.asarray(ids, np.int64)))
    if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise FrtError("instance ids must be a flat list of unsigned 32-bit indices")
    return ids.size, ids.astype(np.uint32)


def id_list_args(ids, what):
    """(n, ids) for the *_remove_materials / _meshes / _lights calls: `ids` an int or a sequence."""
    ids = np.ascontiguousarray(np.atleast_1d(np.asarray(ids, np.int64)))
    if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise FrtError(f"{what} ids must be a flat list of unsigned 32-bit indices")
    return ids.size, ids.astype(np.uint32)


def layer_args(kind, layer):
    """(kind, layer) for the *_remove_texture calls: kind 0 / "color" or 1 / "data"."""
    k = {"color": 0, "colour": 0, "data": 1}.get(kind, kind)
    if k not in (0, 1):
        raise ValueError(f'kind must be "color" (0) or "data" (1), not {kind!r}')
    if not 0 <= int(layer) <= 0xFFFFFFFF:
        raise FrtError("layer must be an unsigned 32-bit index")
    return int(k), int(layer)


def emission_args(light, color, intensity):
    if not 0 <= int(light) <= 0xFFFFFFFF:
        raise FrtError("light must be an unsigned 32-bit index")
    c = np.ascontiguousarray(color, np.float32).reshape(-1)
    if c.size != 3:
        raise FrtError("color must hold three values")
    return int(light), c, float(intensity)


def texture_args(kind, layer, rgba8):
    """(kind, layer, pixels) for the *_set_texture calls: kind 0 / "color" or 1 / "data", `rgba8` 1024 x 1024 x 4 bytes."""
    kind = {"color": 0, "colour": 0, "data": 1}.get(kind, kind)
    if not 0 <= int(layer) <= 0xFFFFFFFF:
        raise FrtError("layer must be an unsigned 32-bit index")
    t = np.ascontiguousarray(rgba8, np.uint8)
    if t.size != 1024 * 1024 * 4:
        raise FrtError("a texture layer is 1024 x 1024 RGBA8")
    return int(kind), int(layer), t


# ---- the calls that add meshes, materials, texture layers and lights to a renderer's replica (include/frt.h: frt_renderer_add_meshes ...; DESIGN.md
# section 15). A wrong shape or dtype is a ValueError here, before the library sees anything.
def _exact(a, dtype, what):
    """`a` as a contiguous array of `dtype`; an array of another kind (floats for indices, integers for pixels) is refused, not converted."""
    a = np.asarray(a)
    want = np.dtype(dtype)
    if a.dtype != want and not (a.dtype.kind in "iu" and want.kind in "iu") and not (a.dtype.kind == "f" and want.kind == "f"):
        raise ValueError(f"{what} must be {want.name}, not {a.dtype.name}")
    if a.dtype.kind in "iu" and a.size and (a.min() < 0 or a.max() > np.iinfo(want).max):
        raise ValueError(f"{what} must fit {want.name}")
    return np.ascontiguousarray(a, want)


def mesh_add_args(geometries):
    """(n, frt_mesh_data array, the arrays it points into) for the *_add_meshes calls: anything with .positions [v, 4] float, .attributes [v, 8] float
    and .indices [3 t] integer per mesh, as SceneBuilder.add_mesh takes it; one such object or a sequence."""
    if hasattr(geometries, "positions"):
        geometries = [geometries]
    geometries = list(geometries)
    recs, keep = (MeshData * max(len(geometries), 1))(), []
    for k, g in enumerate(geometries):
        pos, att, idx = _exact(g.positions, np.float32, "positions"), _exact(g.attributes, np.float32, "attributes"), _exact(g.indices, np.uint32, "indices")
        if pos.ndim != 2 or pos.shape[1] != 4:
            raise ValueError(f"mesh {k}: positions must be shaped [n, 4]")
        if att.size != pos.shape[0] * 8:
            raise ValueError(f"mesh {k}: {pos.shape[0]} positions but {att.size / 8:g} attribute records of 8 floats")
        if idx.ndim != 1:
            raise ValueError(f"mesh {k}: indices must be a flat array")
        keep.append((pos, att, idx))
        recs[k] = MeshData(pos.ctypes.data, att.ctypes.data, idx.ctypes.data, pos.shape[0], idx.size)
    return len(geometries), recs, keep


def material_add_args(materials):
    """(n, [n, 16] uint32 records) for the *_add_materials calls: one frt.Material (or a 64-byte row of get("materials")) or a sequence of them."""
    if isinstance(materials, Material):
        materials = [materials]
    rows = []
    for m in materials:
        r = np.frombuffer(bytes(m), np.uint32) if isinstance(m, Material) else np.ascontiguousarray(m).view(np.uint32).reshape(-1)
        if r.size != 16:
            raise ValueError("a material is 64 bytes")
        rows.append(r)
    return len(rows), (np.ascontiguousarray(np.stack(rows), np.uint32) if rows else np.zeros((0, 16), np.uint32))


def light_add_args(lights):
    """(n, [n, 16] uint32 records) for the *_add_lights calls: one frt.Light (or a 64-byte row of get("lights")) or a sequence of them."""
    if isinstance(lights, Light):
        lights = [lights]
    rows = []
    for l in lights:
        r = np.frombuffer(bytes(l), np.uint32) if isinstance(l, Light) else np.ascontiguousarray(l).view(np.uint32).reshape(-1)
        if r.size != 16:
            raise ValueError("a light is 64 bytes")
        rows.append(r)
    return len(rows), (np.ascontiguousarray(np.stack(rows), np.uint32) if rows else np.zeros((0, 16), np.uint32))


def texture_add_args(kind, rgba8):
    """(kind, pixels) for the *_add_texture calls: kind 0 / "color" or 1 / "data", `rgba8` 1024 x 1024 x 4 bytes of uint8."""
    k = {"color": 0, "colour": 0, "data": 1}.get(kind, kind)
    if k not in (0, 1):
        raise ValueError(f'kind must be "color" (0) or "data" (1), not {kind!r}')
    t = np.asarray(rgba8)
    if t.dtype != np.uint8:
        raise ValueError(f"a texture layer is uint8, not {t.dtype.name}")
    if t.size != 1024 * 1024 * 4:
        raise ValueError("a texture layer is 1024 x 1024 RGBA8")
    return int(k), np.ascontiguousarray(t)


def light_register_args(mesh_id, transform_colmajor, color, intensity):
    """(mesh id, matrix, colour, intensity) for the *_register_quad_light / _sphere_light calls."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise ValueError("mesh id must be an unsigned 32-bit index")
    m = np.ascontiguousarray(transform_colmajor, np.float32).reshape(-1)
    c = np.ascontiguousarray(color, np.float32).reshape(-1)
    if m.size != 16:
        raise ValueError("the transform is one column-major 4x4")
    if c.size != 3:
        raise ValueError("color must hold three values")
    return int(mesh_id), m, c, float(intensity)


def gltf_layer_plan(model, color_layers, data_layers):
    """What SceneBuilder.add_gltf_materials would add to a scene with that many texture layers (include/frt.h: frt_model_layer_plan; the library's own
    remapping): (materials with their slots remapped to layer ids, images that become the next colour layers, images that become the next data layers)."""
    n = model.counts()
    mats = np.zeros((max(n["materials"], 1), 16), np.uint32)
    ci, di, c = np.zeros(max(n["images"], 1), np.uint32), np.zeros(max(n["images"], 1), np.uint32), (C.c_uint32 * 2)()
    check(lib().frt_model_layer_plan(model._h, color_layers, data_layers, mats.ctypes.data, ci.ctypes.data, di.ctypes.data, c))
    return mats[:n["materials"]], [int(i) for i in ci[:c[0]]], [int(i) for i in di[:c[1]]]


HIT_FIELDS = ("t", "u", "v", "tri", "instance", "material", "primitive", "front")      # include/frt.h: frt_ray_hit, one 32-bit word each


def ray_args(origins, dirs, tmin, tmax):
    """The [n, 8] float32 ray records (include/frt.h: frt_ray) of the *_trace_* calls: `origins` and `dirs` shaped [n, 3] (or [3]), `tmin` / `tmax`
    scalars or one value per ray."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise FrtError(f"{o.shape[0]} ray origins but {d.shape[0]} directions")
    rays = np.empty((o.shape[0], 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 4:7] = d
    try:
        rays[:, 3] = np.asarray(tmin, np.float32)
        rays[:, 7] = np.asarray(tmax, np.float32)
    except ValueError:
        raise FrtError("tmin / tmax must be scalars or hold one value per ray") from None
    return rays


def hits_dict(raw):
    """An [n, 8] uint32 array of frt_ray_hit records as a dict of arrays: t, u, v float32; tri (0xFFFFFFFF = miss), instance, material, primitive,
    front uint32."""
    f = raw.view(np.float32)
    return {name: (f if k < 3 else raw)[:, k].copy() for k, name in enumerate(HIT_FIELDS)}


def pixel_args(xy, width, height):
    p = np.asarray(xy, np.int64).reshape(-1, 2)
    if p.size and (p.min() < 0 or p.max() > 0xFFFFFFFF):
        raise FrtError("pixel coordinates must be unsigned 32-bit integers")
    return np.ascontiguousarray(p.astype(np.uint32))


class SceneBuilder:
    def __init__(self, handle=None):
        self._destroy = lib().frt_scene_destroy
        self._h = handle if handle is not None else lib().frt_scene_create()
        if not self._h:
            raise FrtError("scene creation failed: " + lib().frt_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)     # bound at construction: module globals may already be gone at interpreter exit
            self._h = None

    # builder.rs:123
    def add_mesh(self, geo):
        pos = np.ascontiguousarray(geo.positions, np.float32)
        att = np.ascontiguousarray(geo.attributes, np.float32)
        idx = np.ascontiguousarray(geo.indices, np.uint32)
        return check(lib().frt_scene_add_mesh(self._h, pos.ctypes.data, pos.shape[0], att.ctypes.data, idx.ctypes.data, idx.size))

    # builder.rs:117
    def add_material(self, mat):
        return check(lib().frt_scene_add_material(self._h, C.byref(mat)))

    # builder.rs:181 (the mask argument is ignored by the reference as well)
    def add_instance(self, mesh_id, mat_id, transform_colmajor, _mask=0x1):
        m = np.ascontiguousarray(transform_colmajor, np.float32).reshape(16)
        return check(lib().frt_scene_add_instance(self._h, mesh_id, mat_id, m.ctypes.data))

    def add_light(self, light):
        return check(lib().frt_scene_add_light(self._h, C.byref(light)))

    # builder.rs:316 / :353
    def register_quad_light(self, mesh_id, transform_colmajor, color, intensity):
        m = np.ascontiguousarray(transform_colmajor, np.float32).reshape(16)
        c = np.asarray(color, np.float32)
        return check(lib().frt_scene_register_quad_light(self._h, mesh_id, m.ctypes.data, c.ctypes.data, float(intensity)))

    def register_sphere_light(self, mesh_id, transform_colmajor, color, intensity):
        m = np.ascontiguousarray(transform_colmajor, np.float32).reshape(16)
        c = np.asarray(color, np.float32)
        return check(lib().frt_scene_register_sphere_light(self._h, mesh_id, m.ctypes.data, c.ctypes.data, float(intensity)))

    # builder.rs:93 / :105
    def add_color_texture(self, rgba8):
        t = np.ascontiguousarray(rgba8, np.uint8).reshape(1024, 1024, 4)
        return check(lib().frt_scene_add_texture(self._h, 0, t.ctypes.data))

    def add_data_texture(self, rgba8):
        t = np.ascontiguousarray(rgba8, np.uint8).reshape(1024, 1024, 4)
        return check(lib().frt_scene_add_texture(self._h, 1, t.ctypes.data))

    # builder.rs:191-292 / :294-300 / :302-314 — `model` is a frt.loader.Model
    def add_gltf_materials(self, model):
        ids = np.zeros(max(model.counts()["materials"], 1), np.uint32)
        n = check(lib().frt_scene_add_gltf_materials(self._h, model._h, ids.ctypes.data))
        return ids[:n].copy()

    def add_gltf_meshes(self, model):
        ids = np.zeros(max(model.counts()["geometries"], 1), np.uint32)
        n = check(lib().frt_scene_add_gltf_meshes(self._h, model._h, ids.ctypes.data))
        return ids[:n].copy()

    def add_gltf_instances(self, model, mesh_ids, mat_ids, transform_colmajor):
        me = np.ascontiguousarray(mesh_ids, np.uint32); ma = np.ascontiguousarray(mat_ids, np.uint32)
        m = np.ascontiguousarray(transform_colmajor, np.float32).reshape(16)
        return check(lib().frt_scene_add_gltf_instances(self._h, model._h, me.ctypes.data, me.size, ma.ctypes.data, ma.size, m.ctypes.data))

    # builder.rs:431
    def build(self):
        check(lib().frt_scene_build(self._h))
        return self

    # Move instances of the built scene: same tree, refit boxes (include/frt.h: frt_scene_set_instance_transforms). Host copy only.
    def set_instance_transforms(self, ids, transforms_colmajor):
        n, i, m = transform_args(ids, transforms_colmajor)
        check(lib().frt_scene_set_instance_transforms(self._h, n, i.ctypes.data, m.ctypes.data))
        return self

    def set_instance_transform(self, instance_id, transform_colmajor):
        return self.set_instance_transforms([instance_id], [transform_colmajor])

    # Deform one mesh of the built scene: same topology and tree, refit boxes (include/frt.h: frt_scene_set_mesh_vertices). Host copy only.
    # normals="recompute": the vertex normals are computed from the new positions (frt_scene_set_mesh_vertices_ex, FRT_DEFORM_RECOMPUTE_NORMALS).
    def set_mesh_vertices(self, mesh_id, positions, attributes=None, normals="keep"):
        set_mesh_vertices_call("frt_scene_set_mesh_vertices", self._h, mesh_id, positions, attributes, normals)
        return self

    # Linear-blend skinning (include/frt.h: frt_scene_set_mesh_skin, frt_scene_set_mesh_pose). set_mesh_skin binds four joints and four weights per vertex;
    # the mesh's positions at the call become the bind pose (joints=None removes the skin; num_joints defaults to the largest index + 1). set_mesh_pose
    # skins the bind pose under one column-major 4x4 per joint and applies the result as set_mesh_vertices does. Host copy only.
    # mode="dual_quaternion" (frt_scene_set_mesh_skin_ex, FRT_SKIN_DUAL_QUATERNION) binds the mesh to be posed by the dual-quaternion blend instead.
    def set_mesh_skin(self, mesh_id, joints, weights=None, num_joints=None, mode="linear"):
        set_mesh_skin_call("frt_scene_set_mesh_skin", self._h, mesh_id, joints, weights, _num_joints(joints, num_joints), mode)
        return self

    # morph_weights: morph first, then skin the morphed positions (frt_scene_set_mesh_pose_ex); None is the plain pose.
    def set_mesh_pose(self, mesh_id, joint_matrices, normals="recompute", morph_weights=None):
        set_mesh_pose_call("frt_scene_set_mesh_pose", self._h, mesh_id, joint_matrices, normals, morph_weights)
        return self

    # Several meshes under one palette and/or one weight vector, all or nothing (include/frt.h: frt_scene_set_mesh_poses): a palette only skins, weights
    # only morph, both morph then skin; the result is that of the single calls in the order of `mesh_ids`. Host copy only.
    def set_mesh_poses(self, mesh_ids, joint_matrices=None, morph_weights=None, normals="recompute"):
        set_mesh_poses_call("frt_scene_set_mesh_poses", self._h, mesh_ids, joint_matrices, morph_weights, normals)
        return self

    # An animated pose ("Animation"): `rig` (frt.Rig) evaluated at clip `clip`, time `t`, then set_mesh_poses on the host copy.
    def animate(self, rig, mesh_ids, clip, t, normals="recompute"):
        return self.set_mesh_poses(mesh_ids, *rig.evaluate(clip, t), normals=normals)

    # Node animation ("Node animation"): rig.evaluate_nodes, then set_instance_transforms on the host copy.
    def animate_instances(self, rig, instance_ids, nodes, clip, t, root=None, offsets=None):
        return self.set_instance_transforms(instance_ids, rig.evaluate_nodes(clip, t, nodes, root, offsets))

    # A whole cast ("Animating a cast"): the host form of Renderer.animate_cast. An entry is the arguments of animate,
    # (rig, mesh_ids, clip, t), or of animate_instances, (rig, instance_ids, nodes, clip, t[, root[, offsets]]), or a dict of them by name; the
    # instance entries are applied first, then the mesh entries, through those two calls.
    def animate_cast(self, entries, normals="recompute"):
        from .animation import host_cast
        host_cast(self, entries, normals)
        return self

    # Blending clips ("Blending clips"): the three calls above with `samples`, [(clip, t, weight), ...], where they take a clip
    # and a time: rig.evaluate_blend / rig.evaluate_nodes_blend on the host, then the same host calls.
    def animate_blend(self, rig, mesh_ids, samples, normals="recompute"):
        return self.set_mesh_poses(mesh_ids, *rig.evaluate_blend(samples), normals=normals)

    def animate_instances_blend(self, rig, instance_ids, nodes, samples, root=None, offsets=None):
        return self.set_instance_transforms(instance_ids, rig.evaluate_nodes_blend(samples, nodes, root, offsets))

    def animate_cast_blend(self, entries, normals="recompute"):
        from .animation import host_cast_blend
        host_cast_blend(self, entries, normals)
        return self

    # Layering clips ("Layering clips"): the host forms of Renderer.animate_layers, animate_instances_layers and
    # animate_cast_layers: rig.evaluate_layers / rig.evaluate_nodes_layers on the host under `masks`, then the same host calls.
    # goals= and targets= ("Inverse kinematics", "Chain IK"): frt.TwoBone / frt.Aim / frt.Chain and their [G, 8] target rows, applied to the layered pose on the host.
    def animate_layers(self, rig, mesh_ids, layers, masks=None, normals="recompute", goals=None, targets=None):
        return self.set_mesh_poses(mesh_ids, *rig.evaluate_layers(layers, masks, goals, targets), normals=normals)

    def animate_instances_layers(self, rig, instance_ids, nodes, layers, masks=None, root=None, offsets=None, goals=None, targets=None):
        return self.set_instance_transforms(instance_ids, rig.evaluate_nodes_layers(layers, nodes, root, offsets, masks, goals, targets))

    def animate_cast_layers(self, entries, normals="recompute"):
        from .animation import host_cast_layers
        host_cast_layers(self, entries, normals)
        return self

    # Morph targets (include/frt.h: frt_scene_set_mesh_morph_targets, frt_scene_set_mesh_morph_weights). set_mesh_morph_targets binds `deltas` [T, n, 3]
    # float32; the mesh's positions at the call become the base (deltas=None removes the targets). set_mesh_morph_weights adds the weighted deltas to the
    # base in target order and applies the result as set_mesh_vertices does. Host copy only.
    def set_mesh_morph_targets(self, mesh_id, deltas):
        set_mesh_morph_targets_call("frt_scene_set_mesh_morph_targets", self._h, mesh_id, deltas)
        return self

    def set_mesh_morph_weights(self, mesh_id, weights, normals="recompute"):
        set_mesh_morph_weights_call("frt_scene_set_mesh_morph_weights", self._h, mesh_id, weights, normals)
        return self

    # ---- what the built scene looks like (include/frt.h: frt_scene_set_materials and the three calls after it). Host copy only.
    def set_materials(self, ids, materials):
        n, i, m = material_args(ids, materials)
        check(lib().frt_scene_set_materials(self._h, n, i.ctypes.data, m.ctypes.data))
        return self

    def set_instance_materials(self, instance_ids, material_ids):
        n, i, m = id_pair_args(instance_ids, material_ids)
        check(lib().frt_scene_set_instance_materials(self._h, n, i.ctypes.data, m.ctypes.data))
        return self

    def set_light_emission(self, light, color, intensity):
        l, c, i = emission_args(light, color, intensity)
        check(lib().frt_scene_set_light_emission(self._h, l, c.ctypes.data, i))
        return self

    def set_texture(self, kind, layer, rgba8):
        k, l, t = texture_args(kind, layer, rgba8)
        check(lib().frt_scene_set_texture(self._h, k, l, t.ctypes.data))
        return self

    # ---- how many instances the built scene holds (include/frt.h: frt_scene_add_instances / _remove_instances). Host copy only:
    # each costs a host build and leaves the scene equal to one built from scratch with the resulting instance list.
    def add_instances(self, mesh_ids, mat_ids, transforms_colmajor):
        """Append instances of existing meshes and materials; returns the id of the first new instance."""
        n, me, ma, m = instance_add_args(mesh_ids, mat_ids, transforms_colmajor)
        return check(lib().frt_scene_add_instances(self._h, n, me.ctypes.data, ma.ctypes.data, m.ctypes.data))

    def remove_instances(self, ids):
        """Remove instances (an id given twice once); the ids above them shift down."""
        n, i = instance_id_args(ids)
        check(lib().frt_scene_remove_instances(self._h, n, i.ctypes.data))
        return self

    # ---- what the built scene no longer holds (include/frt.h: frt_scene_remove_materials and the three calls after it). Host copy
    # only: ids stay dense (those above a removed one shift down), and the scene equals one built from scratch with the surviving builder calls.
    def remove_materials(self, ids):
        """Remove materials no instance uses; the material ids above them shift down."""
        n, i = id_list_args(ids, "material")
        check(lib().frt_scene_remove_materials(self._h, n, i.ctypes.data))
        return self

    def remove_meshes(self, ids):
        """Remove meshes no instance uses; the mesh ids above them shift down and the vertex and index lists close up."""
        n, i = id_list_args(ids, "mesh")
        check(lib().frt_scene_remove_meshes(self._h, n, i.ctypes.data))
        return self

    def remove_lights(self, ids):
        """Remove lights: an add_light light loses its record, a registered light leaves with its instance and its emissive material."""
        n, i = id_list_args(ids, "light")
        check(lib().frt_scene_remove_lights(self._h, n, i.ctypes.data))
        return self

    def remove_texture(self, kind, layer):
        """Remove one texture layer no material names: kind "color" (0) or "data" (1); the layers above it shift down."""
        k, l = layer_args(kind, layer)
        check(lib().frt_scene_remove_texture(self._h, k, l))
        return self

    # ---- ray queries on the host copy of the built scene (include/frt.h: frt_scene_trace_closest / _any): the specification of Renderer.trace_*
    def trace_closest(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        """Closest hit of every ray origin + t * dir, tmin < t < tmax: a dict of arrays (t, u, v, tri, instance, material, primitive, front);
        tri == 0xFFFFFFFF is a miss (t = -1, the other fields 0)."""
        rays = ray_args(origins, dirs, tmin, tmax)
        out = np.zeros((rays.shape[0], 8), np.uint32)
        check(lib().frt_scene_trace_closest(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data))
        return hits_dict(out)

    def trace_any(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        """Is the segment blocked? A bool per ray: some triangle is hit at tmin < t < tmax."""
        rays = ray_args(origins, dirs, tmin, tmax)
        out = np.zeros(rays.shape[0], np.uint8)
        check(lib().frt_scene_trace_any(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data))
        return out.astype(bool)

    # ---- introspection
    def counts(self):
        c = (C.c_uint32 * 8)()
        check(lib().frt_scene_counts(self._h, c))
        return dict(zip(("tris", "instances", "materials", "lights", "meshes", "attributes", "indices", "bvh2_nodes"), list(c)))

    @property
    def num_lights(self):
        return self.counts()["lights"]

    def tree_stats(self):
        s = (C.c_uint32 * 8)()
        check(lib().frt_scene_tree_stats(self._h, s))
        return dict(zip(("quad_nodes", "quad_stack_need", "wide8_nodes", "wide8_stack_need", "wide8_depth", "wide8_children", "wide8_tri_slots", "quad_fold"), list(s)))

    def get(self, what):
        n = self.counts()
        if what in ("quad_nodes", "wide8_nodes", "tri_slots8", "tri_slots"):
            t = self.tree_stats()
            which, shape, dt = {"quad_nodes": (10, (t["quad_nodes"], 32), np.float32), "wide8_nodes": (11, (t["wide8_nodes"], 32), np.uint32),
                                "tri_slots8": (12, (t["wide8_tri_slots"], 12), np.float32), "tri_slots": (13, (n["tris"], 12), np.float32)}[what]
            out = np.zeros(shape, dt)
            check(lib().frt_scene_get(self._h, which, out.ctypes.data))
            return out
        spec = {"tris": (0, (n["tris"], 9), np.float32), "tri_instance": (1, (n["tris"],), np.uint32),
                "materials": (2, (n["materials"], 16), np.uint32), "lights": (3, (n["lights"], 16), np.uint32),
                "attributes": (4, (n["attributes"], 8), np.float32), "indices": (5, (n["indices"],), np.uint32),
                "mesh_infos": (6, (n["meshes"], 4), np.uint32), "instances": (7, (n["instances"], 30), np.uint32),
                "bvh2_nodes": (8, (n["bvh2_nodes"], 8), np.uint32), "bvh2_tri_index": (9, (n["tris"],), np.uint32),
                "pair_nodes": (15, (self.bvh_stats()["pair_nodes"], 16), np.float32), "instances_dev": (16, (n["instances"], 16), np.uint32),
                "shade_tris": (17, (n["tris"], 32), np.float32)}[what]
        out = np.zeros(spec[1], spec[2])
        check(lib().frt_scene_get(self._h, spec[0], out.ctypes.data))
        return out

    def bvh_stats(self):
        s = (C.c_uint32 * 4)()
        check(lib().frt_scene_bvh_stats(self._h, s))
        return dict(zip(("depth", "leaves", "max_leaf", "pair_nodes"), list(s)))
