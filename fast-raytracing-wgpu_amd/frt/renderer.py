"""Renderer mirror (src/renderer.rs) over frt_renderer_*. Every pixel is produced by the HIP kernels in libfrt.so."""
import ctypes as C
import numpy as np
from ._lib import (lib, check, FrtError, RenderOpts, Stats, CameraUniform, BUF_BPP, BUF_ACCUM, BUF_DISPLAY, PHASE_ALL, FLAG_USE_STREAM, QUERY_DEVICE, DEFORM_DEVICE, TRANSFORM_DEVICE)
from .scene import (transform_args, set_mesh_vertices_call, set_mesh_skin_call, set_mesh_pose_call, set_mesh_poses_call, pose_batch_ids, set_mesh_morph_targets_call, set_mesh_morph_weights_call, _num_joints, deform_flags, material_args, id_pair_args, instance_add_args, instance_id_args, emission_args, texture_args, ray_args, hits_dict,
                    pixel_args, HIT_FIELDS, mesh_add_args, material_add_args, light_add_args, texture_add_args, light_register_args, gltf_layer_plan, id_list_args, layer_args)


REBUILD_MODES = {"morton": 0, "sah": 1}      # include/frt.h: FRT_REBUILD_MORTON, FRT_REBUILD_SAH


def rebuild_mode(quality):
    if quality not in REBUILD_MODES:
        raise ValueError(f"rebuild_tree: quality must be one of {sorted(REBUILD_MODES)}, not {quality!r}")
    return REBUILD_MODES[quality]


def _is_device_tensor(x):
    """A torch tensor in device memory (torch is only imported by callers that pass one)."""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "is_cuda") and x.is_cuda


def _mesh_id(mesh_id):
    """`mesh_id` as the unsigned 32-bit index the C calls take, or FrtError."""
    if not 0 <= int(mesh_id) <= 0xFFFFFFFF:
        raise FrtError("mesh id must be an unsigned 32-bit index")
    return int(mesh_id)


def device_transform_args(torch, ids, mats, device):
    """The record count of a device-tensor set_instance_transforms call on HIP device `device`, or FrtError: `ids` contiguous int32 [n], `mats`
    contiguous float32 [n, 16] or [n, 4, 4] (column-major, as the host form), both on that device. Looks at the tensors' descriptions only."""
    for name, t in (("ids", ids), ("matrices", mats)):
        if t.device.index != device:
            raise FrtError(f"set_instance_transforms: {name} are on {t.device}, the renderer on device {device}")
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise FrtError("set_instance_transforms: device ids must be a contiguous int32 tensor shaped [n]")
    shape = tuple(mats.shape)
    if mats.dtype != torch.float32 or not (shape[1:] == (16,) or shape[1:] == (4, 4)) or len(shape) < 2 or not mats.is_contiguous():
        raise FrtError("set_instance_transforms: device matrices must be a contiguous float32 tensor shaped [n, 16] or [n, 4, 4]")
    if shape[0] != ids.shape[0]:
        raise FrtError(f"{ids.shape[0]} instance ids but {shape[0]} matrices")
    return int(ids.shape[0])


class _HostQueries:
    """trace_closest / trace_any / pick over a handle's host-pointer entry points (numpy in, numpy out); Renderer and MultiRenderer name theirs."""
    _trace_closest = _trace_any = _pick = None

    def _host_trace_closest(self, origins, dirs, tmin, tmax):
        rays = ray_args(origins, dirs, tmin, tmax)
        out = np.zeros((rays.shape[0], 8), np.uint32)
        check(getattr(lib(), self._trace_closest)(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data, 0))
        return hits_dict(out)

    def _host_trace_any(self, origins, dirs, tmin, tmax):
        rays = ray_args(origins, dirs, tmin, tmax)
        out = np.zeros(rays.shape[0], np.uint8)
        check(getattr(lib(), self._trace_any)(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data, 0))
        return out.astype(bool)

    def _host_pick(self, camera_uniform, xy):
        p = pixel_args(xy, self.width, self.height)
        out = np.zeros((p.shape[0], 8), np.uint32)
        check(getattr(lib(), self._pick)(self._h, C.byref(camera_uniform), p.shape[0], p.ctypes.data, out.ctypes.data, 0))
        return hits_dict(out)


def _hit_views(hits):
    """Named views of an [n, 8] int32 tensor of frt_ray_hit records (no copies, no kernels beyond torch's view bookkeeping)."""
    import torch
    f = hits.view(torch.float32)
    d = {"hits": hits}
    for k, name in enumerate(HIT_FIELDS):
        d[name] = (f if k < 3 else hits)[:, k]
    return d


class _SceneGrowth:
    """New meshes, materials, texture layers and lights for the scene replica(s) of a running renderer (include/frt.h: frt_renderer_add_meshes and the
    calls after it): between frames, the arguments copied during the call; accumulation, reservoirs and frame_count are kept. The
    new ids are accepted at once by add_instances and the set_* edits; pass the new light count to build_uniform from the next frame on. The host scene
    is not changed (its route is SceneBuilder.add_* followed by build()). Renderer and MultiRenderer name their entry points in `_grow`."""
    _grow = None

    def _grow_call(self, name, *args):
        return check(getattr(lib(), self._grow + name)(self._h, *args))

    def add_meshes(self, geometries):
        """Append meshes (one or a sequence of objects with .positions / .attributes / .indices); returns the id of the first new mesh."""
        n, recs, _keep = mesh_add_args(geometries)
        return self._grow_call("add_meshes", n, C.cast(recs, C.c_void_p))

    def add_materials(self, materials):
        """Append materials (they may name layers and lights added before); returns the id of the first new material."""
        n, m = material_add_args(materials)
        return self._grow_call("add_materials", n, m.ctypes.data)

    def add_texture(self, kind, rgba8):
        """Append one texture layer: kind "color" (0) or "data" (1), rgba8 1024 x 1024 x 4 bytes; returns its layer id."""
        k, t = texture_add_args(kind, rgba8)
        return self._grow_call("add_texture", k, t.ctypes.data)

    def add_lights(self, lights):
        """Append light records as SceneBuilder.add_light takes them (no instance, no link); returns the index of the first new light."""
        n, l = light_add_args(lights)
        return self._grow_call("add_lights", n, l.ctypes.data)

    def register_quad_light(self, mesh_id, transform_colmajor, color, intensity, quality="sah"):
        """SceneBuilder.register_quad_light on the replica: an emissive material, an instance of `mesh_id` and a light linked to it, then the device
        tree rebuild `quality` names (synchronous). Returns the light index."""
        me, m, c, i = light_register_args(mesh_id, transform_colmajor, color, intensity)
        return self._grow_call("register_quad_light", me, m.ctypes.data, c.ctypes.data, i, rebuild_mode(quality))

    def register_sphere_light(self, mesh_id, transform_colmajor, color, intensity, quality="sah"):
        me, m, c, i = light_register_args(mesh_id, transform_colmajor, color, intensity)
        return self._grow_call("register_sphere_light", me, m.ctypes.data, c.ctypes.data, i, rebuild_mode(quality))


    # ---- and out again (include/frt.h: frt_renderer_remove_materials and the three calls after it): ids stay dense, those above a
    # removed one shift down, and the material id every pixel keeps in BUF_GPOS.w follows (65535.0 where the material left).
    def remove_materials(self, ids):
        """Remove materials no instance uses from the replica(s)."""
        n, i = id_list_args(ids, "material")
        self._grow_call("remove_materials", n, i.ctypes.data)

    def remove_meshes(self, ids):
        """Remove meshes no instance uses from the replica(s); the vertex and index pools close up."""
        n, i = id_list_args(ids, "mesh")
        self._grow_call("remove_meshes", n, i.ctypes.data)

    def remove_lights(self, ids, quality="sah"):
        """Remove lights from the replica(s): an add_lights light loses its record; a registered light leaves with its instance and its emissive material,
        which ends in the device tree rebuild `quality` names (synchronous). Pass the new light count to build_uniform from the next frame on."""
        n, i = id_list_args(ids, "light")
        self._grow_call("remove_lights", n, i.ctypes.data, rebuild_mode(quality))

    def remove_texture(self, kind, layer):
        """Remove one texture layer no material names: kind "color" (0) or "data" (1); the layers above it shift down."""
        k, l = layer_args(kind, layer)
        self._grow_call("remove_texture", k, l)


class Renderer(_HostQueries, _SceneGrowth):
    _trace_closest, _trace_any, _pick = "frt_renderer_trace_closest", "frt_renderer_trace_any", "frt_renderer_pick"
    _grow = "frt_renderer_"

    def __init__(self, scene, width, height, max_depth=8, device=0, stream=None, rows=None, arena=None, arena_bytes=0, flags=0, motion_halo=0,
                 queue_capacity=0, cuts=None):
        """Renderer::new (renderer.rs:206). rows=(begin,end) restricts this renderer to an image strip; motion_halo = rows of
        previous-frame state kept valid beyond the strip for a moving camera (frt.dist.StripPlan(motion_halo=...))."""
        o = RenderOpts()
        o.max_depth, o.device, o.flags, o.queue_capacity = max_depth, device, flags, queue_capacity
        if cuts is not None:        # frt_render_opts.cut_depths: [] = never cut
            c = list(cuts)[:4] or [0xFFFFFFFF]
            for k, v in enumerate(c):
                o.cut_depths[k] = v
        if stream is not None:      # a caller-owned stream handle; 0 is the legacy default stream (torch's default current stream)
            o.stream = stream or None
            o.flags |= FLAG_USE_STREAM
        if rows is not None:
            o.row_begin, o.row_end = rows
            o.motion_halo_rows = motion_halo
        if arena is not None:
            o.device_arena, o.arena_bytes = arena, arena_bytes
        self.width, self.height = width, height
        self.device = device
        self._scene = scene     # keep the scene alive
        self._held = []         # device tensors of set_mesh_vertices / set_instance_transforms calls the stream may not have passed yet: (event behind the call, tensors)
        self._destroy = lib().frt_renderer_destroy
        self._h = lib().frt_renderer_create(scene._h, width, height, C.byref(o))
        if not self._h:
            raise FrtError("renderer creation failed: " + lib().frt_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)     # bound at construction: module globals may already be gone at interpreter exit
            self._h = None

    @staticmethod
    def arena_bytes(width, height):
        return int(lib().frt_renderer_arena_bytes(width, height))

    def aspect_ratio(self):      # renderer.rs:202
        return self.width / self.height

    @property
    def frame_count(self):       # renderer.rs:198
        return int(lib().frt_renderer_frame_count(self._h))

    def render(self, camera_uniform, jitter=None):      # renderer.rs:349 (jitter -> PostParams.jitter, :361-379)
        self._release_held()
        if jitter is None:
            check(lib().frt_renderer_render(self._h, C.byref(camera_uniform)))
        else:
            check(lib().frt_renderer_render_jittered(self._h, C.byref(camera_uniform), float(jitter[0]), float(jitter[1])))

    def set_jitter(self, jitter):
        check(lib().frt_renderer_set_jitter(self._h, float(jitter[0]), float(jitter[1])))

    def fence(self):
        """Order the renderer's stream behind its internal second stream (no host wait); call before using buffer_info pointers."""
        check(lib().frt_renderer_fence(self._h))

    def order_edge_stream(self):
        """The edge stream behind the open frame's T-merge, now (frt_renderer_order_edge_stream): for transfers placed in that stream."""
        check(lib().frt_renderer_order_edge_stream(self._h))

    def stream_handle(self, which=0):
        return lib().frt_renderer_stream(self._h, which) or 0

    def render_phases(self, camera_uniform, phases=PHASE_ALL):
        check(lib().frt_renderer_render_phases(self._h, C.byref(camera_uniform), phases))

    def end_frame(self):
        check(lib().frt_renderer_end_frame(self._h))

    def sync(self):
        check(lib().frt_renderer_sync(self._h))
        self._release_held(all_done=True)

    def reset(self):             # state.rs:152 / renderer.rs:346
        check(lib().frt_renderer_reset(self._h))

    def clear(self):
        check(lib().frt_renderer_clear(self._h))

    def read_buffer(self, buf, index=0):
        bpp = BUF_BPP[buf]
        out = np.zeros((self.height, self.width, bpp), np.uint8)
        check(lib().frt_renderer_read_buffer(self._h, buf, index, out.ctypes.data))
        return out

    def read_rows(self, buf, index, y0, y1):
        out = np.zeros((y1 - y0, self.width, BUF_BPP[buf]), np.uint8)
        check(lib().frt_renderer_read_rows(self._h, buf, index, y0, y1, out.ctypes.data))
        return out

    def write_rows(self, buf, index, y0, y1, data):
        data = np.ascontiguousarray(data, np.uint8)
        assert data.size == (y1 - y0) * self.width * BUF_BPP[buf]
        check(lib().frt_renderer_write_rows(self._h, buf, index, y0, y1, data.ctypes.data))

    def read_display(self):
        return self.read_buffer(BUF_DISPLAY)

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(lib().frt_renderer_read_accum(self._h, out.ctypes.data))
        return out

    def buffer_info(self, buf, index=0):
        p, bpp = C.c_void_p(), C.c_uint32()
        check(lib().frt_renderer_buffer_info(self._h, buf, index, C.byref(p), C.byref(bpp)))
        return p.value, bpp.value

    def phase_rows(self):
        r = (C.c_uint32 * 8)()
        check(lib().frt_renderer_phase_rows(self._h, r))
        v = list(r)
        return {"gbuffer": (v[0], v[1]), "temporal": (v[2], v[3]), "spatial": (v[4], v[5]), "post": (v[6], v[7])}

    def set_timing(self, on):
        check(lib().frt_renderer_set_timing(self._h, 1 if on else 0))

    def set_instance_transforms(self, ids, transforms_colmajor):
        """Move instances in this renderer's scene replica between frames (include/frt.h: frt_renderer_set_instance_transforms): asynchronous, on
        the renderer's streams. The host scene is not changed (SceneBuilder.set_instance_transforms is its own call).
        numpy (or array-like) in: the arrays are checked and copied during the call. Torch tensors on the renderer's device in (ids contiguous int32
        [n], matrices contiguous float32 [n, 16] or [n, 4, 4]; not one of each kind): frt_renderer_set_instance_transforms_ex with
        FRT_TRANSFORM_DEVICE, under the rules of the device form of set_mesh_vertices — the renderer's stream waits for the caller's current stream,
        the call is only enqueued, the renderer keeps a reference to the tensors until that stream has passed the call, nothing waits on the host.
        A bad id, a non-finite entry or a singular 3x3 then rejects the whole call on the device: nothing is applied and transform_rejects()
        counts it."""
        dev_in = [_is_device_tensor(x) for x in (ids, transforms_colmajor)]
        if not any(dev_in):
            n, i, m = transform_args(ids, transforms_colmajor)
            return check(lib().frt_renderer_set_instance_transforms(self._h, n, i.ctypes.data, m.ctypes.data))
        if not all(dev_in):
            raise FrtError("set_instance_transforms: ids and matrices must both be host arrays or both be device tensors")
        import torch
        n = device_transform_args(torch, ids, transforms_colmajor, self.device)
        self._device_call(torch, lambda: lib().frt_renderer_set_instance_transforms_ex(self._h, n, ids.data_ptr() if n else None, transforms_colmajor.data_ptr() if n else None,
                                                                                        TRANSFORM_DEVICE), transforms_colmajor, ids)

    def transform_rejects(self):
        """Device-tensor set_instance_transforms calls rejected so far (a bad id, a non-finite entry, a singular 3x3; nothing of them was applied).
        Waits for the renderer's stream."""
        n = C.c_uint32()
        check(lib().frt_renderer_transform_rejects(self._h, C.byref(n)))
        return int(n.value)

    def set_instance_transform(self, instance_id, transform_colmajor):
        self.set_instance_transforms([instance_id], [transform_colmajor])

    def set_mesh_vertices(self, mesh_id, positions, attributes=None, normals="keep"):
        """Deform one mesh in this renderer's scene replica between frames (include/frt.h: frt_renderer_set_mesh_vertices_ex): asynchronous, on the
        renderer's streams. The host scene is not changed (SceneBuilder.set_mesh_vertices is its own call). normals="recompute": the vertex normals
        are computed on the device from the new positions (uv and tangent from `attributes`, or kept).
        numpy (or array-like) in: the arrays are checked and copied during the call. Contiguous float32 torch tensors on the renderer's device in
        (positions [n, 4], attributes [n, 8]; not one of each kind): nothing is copied to the host and nothing waits — the renderer's stream
        (stream_handle(0)) waits for the caller's current stream, the call is enqueued there, and the renderer keeps a reference to the tensors
        until that stream has passed the call (an event behind it, looked at by the next such call, by render() and by sync()), so the caching allocator cannot hand their
        memory out early. (Tensor.record_stream would say the same to the allocator, but it makes the allocator record an event on the renderer's
        stream when the tensor is freed, and a tensor may outlive the renderer that owns that stream.) A non-finite float then rejects the call
        on the device: nothing is applied and deform_rejects() counts it."""
        dev_in = [_is_device_tensor(x) for x in (positions, attributes) if x is not None]
        if not any(dev_in):
            return set_mesh_vertices_call("frt_renderer_set_mesh_vertices", self._h, mesh_id, positions, attributes, normals)
        if not all(dev_in):
            raise FrtError("set_mesh_vertices: positions and attributes must both be host arrays or both be device tensors")
        import torch
        flags = deform_flags(normals) | DEFORM_DEVICE
        mid = _mesh_id(mesh_id)
        for name, t, cols in (("positions", positions, 4), ("attributes", attributes, 8)):
            if t is not None:
                self._check_device_tensor(torch, "set_mesh_vertices", name, t, lambda t: t.dim() == 2 and t.shape[1] == cols, f"[n, {cols}]")
        if attributes is not None and attributes.shape[0] != positions.shape[0]:
            raise FrtError(f"{positions.shape[0]} positions but {attributes.shape[0]} attribute records")
        self._device_call(torch, lambda: lib().frt_renderer_set_mesh_vertices_ex(self._h, mid, positions.data_ptr(), attributes.data_ptr() if attributes is not None else None,
                                                                                  positions.shape[0], flags), positions, attributes)

    def set_mesh_skin(self, mesh_id, joints, weights=None, num_joints=None, mode="linear"):
        """Bind a skin to one mesh of this renderer's scene replica (include/frt.h: frt_renderer_set_mesh_skin): `joints` [n, 4] integers, `weights`
        [n, 4] float32, copied during the call; the replica's positions of the mesh, as the renderer's stream finds them, become the bind pose.
        joints=None removes the skin; num_joints defaults to the largest joint index + 1. mode: "linear", or "dual_quaternion" (frt_renderer_set_mesh_skin_ex,
        FRT_SKIN_DUAL_QUATERNION): every later pose of the mesh blends its joints as rigid transforms. The host scene is not changed."""
        set_mesh_skin_call("frt_renderer_set_mesh_skin",self._h, mesh_id, joints, weights, _num_joints(joints, num_joints), mode)

    def set_mesh_pose(self, mesh_id, joint_matrices, normals="recompute", morph_weights=None):
        """Pose a skinned mesh of this renderer's scene replica between frames (include/frt.h: frt_renderer_set_mesh_pose): one column-major 4x4 per
        joint, [J, 16] or [J, 4, 4]. One kernel skins the bind pose on the device; the result is applied as set_mesh_vertices applies device
        positions. normals="recompute" (the default: a posed mesh lit with its bind-pose normals is wrong) or "keep".
        numpy (or array-like) in: checked and copied during the call. A contiguous float32 torch tensor on the renderer's device in: the protocol of
        the device form of set_mesh_vertices — the renderer's stream waits for the caller's current stream, the call is only enqueued, and the
        renderer keeps a reference to the tensor until that stream has passed the call. A non-finite matrix entry of a device palette, and for
        either kind a pose that overflows, rejects the call on the device: nothing is applied and deform_rejects() counts it.
        morph_weights [T] (frt_renderer_set_mesh_pose_ex): the mesh is morphed from its morph base first and the morphed positions are skinned, in
        two launches. The palette and the weights are then either both tensors or both arrays; None calls exactly what the plain pose calls."""
        dev_in = [_is_device_tensor(x) for x in (joint_matrices, morph_weights) if x is not None]
        if not any(dev_in):
            return set_mesh_pose_call("frt_renderer_set_mesh_pose", self._h, mesh_id, joint_matrices, normals, morph_weights)
        if not all(dev_in):
            raise TypeError("set_mesh_pose: joint matrices and morph weights must both be host arrays or both be device tensors")
        import torch
        flags = deform_flags(normals) | DEFORM_DEVICE
        mid, t, w = _mesh_id(mesh_id), joint_matrices, morph_weights
        self._check_device_tensor(torch, "set_mesh_pose", "joint matrices", t, lambda t: (t.dim() == 2 and t.shape[1] == 16) or (t.dim() == 3 and tuple(t.shape[1:]) == (4, 4)),
                                  "[J, 16] or [J, 4, 4]")
        if w is None:
            return self._device_call(torch, lambda: lib().frt_renderer_set_mesh_pose(self._h, mid, t.data_ptr(), t.shape[0], flags), t)
        self._check_device_tensor(torch, "set_mesh_pose", "morph weights", w, lambda w: w.dim() == 1, "[T]")
        self._device_call(torch, lambda: lib().frt_renderer_set_mesh_pose_ex(self._h, mid, t.data_ptr(), t.shape[0], w.data_ptr(), w.shape[0], flags), t, w)

    def set_mesh_poses(self, mesh_ids, joint_matrices=None, morph_weights=None, normals="recompute"):
        """Pose several meshes of this renderer's scene replica in one call (include/frt.h: frt_renderer_set_mesh_poses): `mesh_ids` (host integers)
        under one palette [J, 16] or [J, 4, 4] and/or one weight vector [T] — a palette only skins, weights only morph, both morph then skin, for
        every mesh alike. The result is that of the single calls in the order given, but the batch is atomic (a pose of any mesh that overflows
        rejects all of it: deform_rejects() counts one), its launches do not multiply with the number of meshes, and the scene extent and the refit
        run once. numpy in, or contiguous float32 torch tensors on the renderer's device under the protocol of set_mesh_pose; the palette and the
        weights are then either both tensors or both arrays."""
        dev_in = [_is_device_tensor(x) for x in (joint_matrices, morph_weights) if x is not None]
        if not any(dev_in):
            return set_mesh_poses_call("frt_renderer_set_mesh_poses", self._h, mesh_ids, joint_matrices, morph_weights, normals)
        if not all(dev_in):
            raise TypeError("set_mesh_poses: joint matrices and morph weights must both be host arrays or both be device tensors")
        import torch
        flags = deform_flags(normals) | DEFORM_DEVICE
        ids, t, w = pose_batch_ids(mesh_ids), joint_matrices, morph_weights
        if t is not None:
            self._check_device_tensor(torch, "set_mesh_poses", "joint matrices", t, lambda t: (t.dim() == 2 and t.shape[1] == 16) or (t.dim() == 3 and tuple(t.shape[1:]) == (4, 4)),
                                      "[J, 16] or [J, 4, 4]")
        if w is not None:
            self._check_device_tensor(torch, "set_mesh_poses", "morph weights", w, lambda w: w.dim() == 1, "[T]")
        self._device_call(torch, lambda: lib().frt_renderer_set_mesh_poses(self._h, ids.size, ids.ctypes.data, t.data_ptr() if t is not None else None, t.shape[0] if t is not None else 0,
                                                                            w.data_ptr() if w is not None else None, w.shape[0] if w is not None else 0, flags),
                          *[x for x in (t, w) if x is not None])

    # ---- animation (include/frt.h: frt_renderer_bind_rig and the three calls after it; DESIGN.md section 11, "Animation")
    def bind_rig(self, rig, mesh_ids):
        """Copy `rig` (frt.Rig) to the renderer's device and remember `mesh_ids`, every one of which already has the skin and / or the morph targets
        the rig implies (set_mesh_skin with the rig's joint count, set_mesh_morph_targets with its target count). Returns the binding animate takes."""
        ids, b = pose_batch_ids(mesh_ids), C.c_uint32()
        check(lib().frt_renderer_bind_rig(self._h, rig._h, ids.ctypes.data, ids.size, C.byref(b)))
        self._rigs = getattr(self, "_rigs", {})
        self._rigs[int(b.value)] = rig      # (for its clip names and counts; the device copy does not depend on it)
        return int(b.value)

    def animate(self, binding, clip, t, normals="recompute"):
        """Pose the binding's meshes under clip `clip` (a number, or a name of the bound rig) at time `t` between frames: one kernel evaluates the clip
        into a palette and weights the renderer owns, bit for bit rig.evaluate(clip, t), and the call goes on as set_mesh_poses with those device
        buffers. The host passes one float; nothing is read back. A pose that overflows rejects on the device: deform_rejects() counts it."""
        check(lib().frt_renderer_animate(self._h, int(binding), self._bound_rig("animate", binding).clip_index(clip), float(t), deform_flags(normals)))

    def _bound_rig(self, call, binding):
        rig = getattr(self, "_rigs", {}).get(int(binding))
        if rig is None:
            raise FrtError(f"{call}: unknown rig binding {binding}")
        return rig

    def read_rig_pose(self, binding):
        """(palette [J, 16] or None, weights [T] or None) as the binding's last animate left them on the device. Waits for the renderer's stream."""
        rig = self._bound_rig("read_rig_pose", binding)
        pal = np.zeros((rig.num_joints, 16), np.float32) if rig.num_joints else None
        w = np.zeros(rig.num_targets, np.float32) if rig.num_targets else None
        check(lib().frt_renderer_read_rig_pose(self._h, int(binding), pal.ctypes.data if pal is not None else None, w.ctypes.data if w is not None else None))
        return pal, w

    def unbind_rig(self, binding):
        """Free the binding's device memory. Waits for the renderer's stream."""
        check(lib().frt_renderer_unbind_rig(self._h, int(binding)))
        getattr(self, "_rigs", {}).pop(int(binding), None)

    # ---- node animation (include/frt.h: frt_renderer_bind_rig_instances and the two calls after it; DESIGN.md section 11, "Node animation")
    def bind_rig_instances(self, rig, instance_ids, nodes, root=None, offsets=None):
        """Copy `rig` (frt.Rig) to the renderer's device and bind instance instance_ids[k] to node nodes[k] (the node numbers the rig was described
        with; for Model.node_rig() the stored indices of Model.geometry_nodes). root [16] and offsets [n, 16], column-major, or None: the instance's
        matrix is (root * global[node]) * offset. Returns the binding animate_instances takes; it shares the numbers of bind_rig."""
        from .animation import node_args
        n, nodes, root, offsets = node_args(nodes, root, offsets)
        n_ids, ids = instance_id_args(instance_ids)
        if n_ids != n:
            raise FrtError(f"bind_rig_instances: {n_ids} instance ids but {n} nodes")
        b = C.c_uint32()
        check(lib().frt_renderer_bind_rig_instances(self._h, rig._h, n, ids.ctypes.data, nodes.ctypes.data, root.ctypes.data if root is not None else None,
                                                    offsets.ctypes.data if offsets is not None else None, C.byref(b)))
        self._rigs = getattr(self, "_rigs", {})
        self._rigs[int(b.value)] = rig
        self._rig_instances = getattr(self, "_rig_instances", {})
        self._rig_instances[int(b.value)] = n
        return int(b.value)

    def animate_instances(self, binding, clip, t):
        """Move the binding's instances under clip `clip` (a number, or a name of the bound rig) at time `t` between frames: one kernel evaluates the
        clip into matrices the renderer owns, bit for bit rig.evaluate_nodes, and the call goes on as set_instance_transforms with device tensors
        (validated on the device, all or nothing: transform_rejects() counts a rejected call). Asynchronous."""
        check(lib().frt_renderer_animate_instances(self._h, int(binding), self._bound_rig("animate_instances", binding).clip_index(clip), float(t)))

    def read_rig_instances(self, binding):
        """float32 [n, 16]: the binding's matrices as the last animate_instances left them. Waits for the renderer's stream."""
        out = np.zeros((getattr(self, "_rig_instances", {}).get(int(binding), 0), 16), np.float32)
        check(lib().frt_renderer_read_rig_instances(self._h, int(binding), out.ctypes.data if out.size else None))
        return out

    # ---- a whole cast (include/frt.h: frt_renderer_animate_cast; DESIGN.md section 11, "Animating a cast")
    def animate_cast(self, entries, normals="recompute"):
        """Animate several bindings of either kind in one call: `entries` is an iterable of (binding, clip, t), a clip a number or a name of the
        bound rig, in any order. One kernel evaluates every entry (one workgroup each); the instance entries are applied first, as one
        set_instance_transforms with device tensors, then the mesh entries as one pose batch, each half all or nothing (transform_rejects() /
        deform_rejects() count a rejected half once); one refit serves the call. Bit for bit what animate_instances for the instance entries
        followed by animate for the mesh entries leave. Asynchronous; the call does not wait for the stream."""
        from ._lib import CastEntry
        rows = [(int(b), self._bound_rig("animate_cast", b).clip_index(clip), float(t)) for b, clip, t in entries]
        table = (CastEntry * max(len(rows), 1))(*[CastEntry(b, c, t, 0) for b, c, t in rows])
        check(lib().frt_renderer_animate_cast(self._h, len(rows), table, deform_flags(normals)))

    # ---- blending clips (include/frt.h: frt_renderer_animate_blend and the two calls after it; DESIGN.md section 11, "Blending clips")
    def animate_blend(self, binding, samples, normals="recompute"):
        """animate() with a blend where it takes a clip and a time: `samples` is [(clip, t, weight), ...] as Rig.evaluate_blend takes them, e.g. a
        cross-fade [("idle", t0, 1 - f), ("walk", t1, f)]. The same kernel; the palette and weights are rig.evaluate_blend(samples) bit for bit."""
        from .animation import sample_table
        n, table = sample_table(self._bound_rig("animate_blend", binding).sample_rows(samples))
        check(lib().frt_renderer_animate_blend(self._h, int(binding), n, table, deform_flags(normals)))

    def animate_instances_blend(self, binding, samples):
        """animate_instances() with a blend: the matrices are rig.evaluate_nodes_blend(samples, ...) bit for bit."""
        from .animation import sample_table
        n, table = sample_table(self._bound_rig("animate_instances_blend", binding).sample_rows(samples))
        check(lib().frt_renderer_animate_instances_blend(self._h, int(binding), n, table))

    def animate_cast_blend(self, entries, normals="recompute"):
        """animate_cast() with a blend per binding: `entries` is an iterable of (binding, samples). Every rule of animate_cast holds: one launch, the
        instance half then the mesh half, each all or nothing, one refit. Bit for bit what animate_instances_blend for the instance entries
        followed by animate_blend for the mesh entries leave."""
        from ._lib import CastBlendEntry
        from .animation import sample_table
        rows, table = [], []
        for b, samples in entries:
            s = self._bound_rig("animate_cast_blend", b).sample_rows(samples)
            table.append(CastBlendEntry(int(b), len(rows), len(s), 0))
            rows += s
        ns, stable = sample_table(rows)
        check(lib().frt_renderer_animate_cast_blend(self._h, len(table), (CastBlendEntry * max(len(table), 1))(*table), ns, stable, deform_flags(normals)))

    # ---- layering clips (include/frt.h: frt_renderer_set_rig_masks and the three calls after it; DESIGN.md section 11, "Layering clips")
    def set_rig_masks(self, binding, masks):
        """Give a binding of either kind its masks: [nmasks, num_nodes] values in [0, 1] in the rig's node order (Rig.mask), one mask [num_nodes], or
        None to clear them. They replace the previous set and take effect in stream order: a call between two animate calls needs no wait."""
        nm, m = self._bound_rig("set_rig_masks", binding)._mask_args(masks)
        check(lib().frt_renderer_set_rig_masks(self._h, int(binding), nm, m.ctypes.data if m is not None else None))

    # ---- inverse kinematics (include/frt.h: frt_renderer_set_rig_goals, _set_rig_goal_targets; DESIGN.md section 11, "Inverse kinematics")
    def set_rig_goals(self, binding, goals):
        """Give a binding of either kind its goals (frt.TwoBone, frt.Aim, frt.Chain; at most MAX_RIG_GOALS; None clears them). They replace the previous set, in
        stream order, and do nothing until set_rig_goal_targets gives them targets. Only the _layers calls apply goals."""
        n, table = self._bound_rig("set_rig_goals", binding)._goal_rows(goals)
        check(lib().frt_renderer_set_rig_goals(self._h, int(binding), n, table))

    def set_rig_goal_targets(self, binding, targets):
        """The targets of the binding's goals, [G, 8] float32 rows of (target xyz, weight, pole xyz, pole flag) in the rig's model space, one per
        goal. numpy (or array-like) in: checked and copied during the call. A contiguous float32 torch tensor on the renderer's device in (e.g.
        built from trace_closest's device output): the protocol of the device form of set_mesh_vertices — the renderer's stream waits for the
        caller's current stream, one device-to-device copy is enqueued, the renderer keeps a reference to the tensor until the stream has passed
        it, nothing waits. A device row with a non-finite word or a weight outside (0, 1] makes the kernel skip that goal. Takes effect in stream
        order."""
        from ._lib import GOAL_TARGETS_DEVICE
        if not _is_device_tensor(targets):
            from .animation import goal_target_rows
            t = goal_target_rows(targets)
            return check(lib().frt_renderer_set_rig_goal_targets(self._h, int(binding), t.shape[0], t.ctypes.data if t.shape[0] else None, 0))
        import torch
        self._check_device_tensor(torch, "set_rig_goal_targets", "targets", targets, lambda t: t.dim() == 2 and t.shape[1] == 8, "[G, 8]")
        self._device_call(torch, lambda: lib().frt_renderer_set_rig_goal_targets(self._h, int(binding), targets.shape[0], targets.data_ptr() if targets.shape[0] else None,
                                                                                  GOAL_TARGETS_DEVICE), targets)

    def animate_layers(self, binding, layers, normals="recompute"):
        """animate() with a stack of layers (frt.Layer, or (clip, t, weight) for a blend layer) as Rig.evaluate_layers takes them; a layer's mask
        names one of the binding's masks (set_rig_masks). E.g. walk, and wave with the arm: [("walk", t, 1.0), Layer("wave", t, mask=0,
        mode="override")]. The palette and weights are rig.evaluate_layers(layers, masks) bit for bit."""
        from .animation import layer_table
        n, table = layer_table(self._bound_rig("animate_layers", binding)._layer_rows(layers))
        check(lib().frt_renderer_animate_layers(self._h, int(binding), n, table, deform_flags(normals)))

    def animate_instances_layers(self, binding, layers):
        """animate_instances() with a stack of layers: the matrices are rig.evaluate_nodes_layers(layers, ..., masks=the binding's) bit for bit."""
        from .animation import layer_table
        n, table = layer_table(self._bound_rig("animate_instances_layers", binding)._layer_rows(layers))
        check(lib().frt_renderer_animate_instances_layers(self._h, int(binding), n, table))

    def animate_cast_layers(self, entries, normals="recompute"):
        """animate_cast() with a stack of layers per binding: `entries` is an iterable of (binding, layers), each under its own binding's masks.
        Every rule of animate_cast holds. Bit for bit what animate_instances_layers for the instance entries followed by animate_layers for the
        mesh entries leave."""
        from ._lib import CastLayersEntry
        from .animation import layer_table
        rows, table = [], []
        for b, layers in entries:
            s = self._bound_rig("animate_cast_layers", b)._layer_rows(layers)
            table.append(CastLayersEntry(int(b), len(rows), len(s), 0))
            rows += s
        nl, ltable = layer_table(rows)
        check(lib().frt_renderer_animate_cast_layers(self._h, len(table), (CastLayersEntry * max(len(table), 1))(*table), nl, ltable, deform_flags(normals)))

    def _check_device_tensor(self, torch, call, name, t, shape_ok, shape):
        """What a call asks of a device tensor it is handed: it lives on the renderer's device and is contiguous float32 of a shape `shape_ok` accepts
        (`shape`: how the message spells that shape)."""
        if t.device.index != self.device:
            raise FrtError(f"{call}: {name} are on {t.device}, the renderer on device {self.device}")
        if t.dtype != torch.float32 or not t.is_contiguous() or not shape_ok(t):
            raise FrtError(f"{call}: device {name} must be a contiguous float32 tensor shaped {shape}")

    def _device_call(self, torch, call, *tensors):
        """The protocol of every call that takes device tensors: the renderer's stream waits for the caller's current stream, `call` (the C call; its
        code is checked) is enqueued there, and the renderer keeps a reference to `tensors` behind an event until that stream has passed the call."""
        dev = tensors[0].device
        s = self._torch_stream(torch, dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        check(call())
        done = torch.cuda.Event()
        done.record(s)
        self._release_held()
        self._held.append((done,) + tensors)

    def set_mesh_morph_targets(self, mesh_id, deltas):
        """Bind morph targets to one mesh of this renderer's scene replica (include/frt.h: frt_renderer_set_mesh_morph_targets): `deltas` [T, n, 3]
        float32, copied during the call; the replica's positions of the mesh, as the renderer's stream finds them, become the base. deltas=None
        removes the targets. The host scene is not changed."""
        set_mesh_morph_targets_call("frt_renderer_set_mesh_morph_targets", self._h, mesh_id, deltas)

    def set_mesh_morph_weights(self, mesh_id, weights, normals="recompute"):
        """Morph a mesh of this renderer's scene replica between frames (include/frt.h: frt_renderer_set_mesh_morph_weights): one weight per bound
        target, [T]. One kernel adds the weighted deltas to the base on the device, in target order; the result is applied as set_mesh_vertices
        applies device positions. normals="recompute" (the default) or "keep".
        numpy (or array-like) in: checked and copied during the call. A contiguous float32 torch tensor on the renderer's device in: the protocol of
        the device palette of set_mesh_pose — the renderer's stream waits for the caller's current stream, the call is only enqueued, and the
        renderer keeps a reference to the tensor until that stream has passed the call. A non-finite device weight, and for either kind a morph
        that overflows, rejects the call on the device: nothing is applied and deform_rejects() counts it."""
        if not _is_device_tensor(weights):
            return set_mesh_morph_weights_call("frt_renderer_set_mesh_morph_weights", self._h, mesh_id, weights, normals)
        import torch
        flags = deform_flags(normals) | DEFORM_DEVICE
        mid = _mesh_id(mesh_id)
        self._check_device_tensor(torch, "set_mesh_morph_weights", "morph weights", weights, lambda w: w.dim() == 1, "[T]")
        self._device_call(torch, lambda: lib().frt_renderer_set_mesh_morph_weights(self._h, mid, weights.data_ptr(), weights.shape[0], flags), weights)

    def _release_held(self, all_done=False):
        """Drop the references to device tensors whose call the stream has passed (all of them after a sync)."""
        if self._held:
            self._held = [] if all_done else [h for h in self._held if not h[0].query()]

    def deform_rejects(self):
        """Device-tensor set_mesh_vertices calls rejected so far for a non-finite float (nothing of them was applied). Waits for the renderer's stream."""
        n = C.c_uint32()
        check(lib().frt_renderer_deform_rejects(self._h, C.byref(n)))
        return int(n.value)

    # ---- what the replica looks like (include/frt.h: frt_renderer_set_materials and the three calls after it): asynchronous,
    # between frames, the arguments copied during the call; accumulation and reservoirs are kept (reset() / clear() to converge to the new look).
    # The host scene is not changed (SceneBuilder has the same four methods).
    def set_materials(self, ids, materials):
        """Material ids[k] of this renderer's scene replica becomes materials[k]."""
        n, i, m = material_args(ids, materials)
        check(lib().frt_renderer_set_materials(self._h, n, i.ctypes.data, m.ctypes.data))

    def set_instance_materials(self, instance_ids, material_ids):
        """Instance instance_ids[k] uses material material_ids[k]; pick and trace_closest report it at once."""
        n, i, m = id_pair_args(instance_ids, material_ids)
        check(lib().frt_renderer_set_instance_materials(self._h, n, i.ctypes.data, m.ctypes.data))

    def set_light_emission(self, light, color, intensity):
        """Light `light` emits (color, intensity); a light registered with an instance also gets that instance's emissive material updated."""
        l, c, i = emission_args(light, color, intensity)
        check(lib().frt_renderer_set_light_emission(self._h, l, c.ctypes.data, i))

    def set_texture(self, kind, layer, rgba8):
        """Replace one existing texture layer: kind "color" (0) or "data" (1), rgba8 1024 x 1024 x 4 bytes."""
        k, l, t = texture_args(kind, layer, rgba8)
        check(lib().frt_renderer_set_texture(self._h, k, l, t.ctypes.data))

    # ---- ray queries against the replica as it is now (include/frt.h: frt_renderer_trace_closest / _trace_any / _pick)
    def _torch_stream(self, torch, dev):
        h = self.stream_handle(0)
        return torch.cuda.ExternalStream(h, device=dev) if h else torch.cuda.default_stream(dev)

    def _device_rays(self, torch, origins, dirs, tmin, tmax):
        dev = origins.device
        o = origins.reshape(-1, 3)
        rays = torch.empty((o.shape[0], 8), dtype=torch.float32, device=dev)
        rays[:, 0:3] = o
        rays[:, 4:7] = torch.as_tensor(dirs, device=dev).reshape(-1, 3)
        rays[:, 3] = tmin if isinstance(tmin, (int, float)) else torch.as_tensor(tmin, dtype=torch.float32, device=dev)
        rays[:, 7] = tmax if isinstance(tmax, (int, float)) else torch.as_tensor(tmax, dtype=torch.float32, device=dev)
        return rays

    def _device_query(self, anchor, build_input, call, out_shape, out_dtype):
        """Enqueue one query on the renderer's main stream behind the caller's current stream (a stream-level wait, no host wait): `build_input`
        makes the input tensor there, `call` gets (n, input pointer, output pointer). Returns the output tensor; reads are the caller's to order."""
        import torch
        dev = anchor.device
        if dev.index != self.device:
            raise FrtError(f"the tensor is on {dev}, the renderer on device {self.device}")
        s = self._torch_stream(torch, dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            inp = build_input(torch)
            n = inp.shape[0]
            out = torch.empty((n,) + out_shape, dtype=getattr(torch, out_dtype), device=dev)
            check(call(n, inp.data_ptr() if n else None, out.data_ptr() if n else None))
        return out

    def trace_closest(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        """Closest hits against the device replica. numpy (or anything array-like) in: synchronous, a dict of numpy arrays as
        SceneBuilder.trace_closest. A torch tensor on the renderer's device in: the rays are assembled on the device, the call is only enqueued on
        the renderer's stream (stream_handle(0)) and the result is a dict of device tensors — "hits", the [n, 8] int32 records, and a view per
        field (t, u, v float32) — that the caller reads behind that stream; nothing waits."""
        if not _is_device_tensor(origins):
            return self._host_trace_closest(origins, dirs, tmin, tmax)
        hits = self._device_query(origins, lambda torch: self._device_rays(torch, origins, dirs, tmin, tmax),
                                  lambda n, i, o: lib().frt_renderer_trace_closest(self._h, n, i, o, QUERY_DEVICE), (8,), "int32")
        return _hit_views(hits)

    def trace_any(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        """Is the segment blocked? numpy in: a bool array; a device tensor in: a bool device tensor, enqueued as trace_closest."""
        if not _is_device_tensor(origins):
            return self._host_trace_any(origins, dirs, tmin, tmax)
        import torch
        occ = self._device_query(origins, lambda torch: self._device_rays(torch, origins, dirs, tmin, tmax),
                                 lambda n, i, o: lib().frt_renderer_trace_any(self._h, n, i, o, QUERY_DEVICE), (), "uint8")
        return occ.view(torch.bool)

    def pick(self, camera_uniform, xy):
        """What is under these pixels? The closest hit of the primary ray of every pixel (x, y) of `xy` ([n, 2]) under `camera_uniform`: the hit the
        G-buffer stage finds there. numpy in: synchronous, a dict of arrays, FrtError for a pixel outside the frame; an integer device tensor in:
        enqueued, a dict of device tensors as trace_closest, a pixel outside the frame a miss."""
        if not _is_device_tensor(xy):
            return self._host_pick(camera_uniform, xy)
        hits = self._device_query(xy, lambda torch: xy.reshape(-1, 2).to(torch.int32).contiguous(),
                                  lambda n, i, o: lib().frt_renderer_pick(self._h, C.byref(camera_uniform), n, i, o, QUERY_DEVICE), (8,), "int32")
        return _hit_views(hits)

    def rebuild_tree(self, quality="morton"):
        """Build a new quad tree over the replica's triangles as they are now, on the device (include/frt.h: frt_renderer_rebuild_tree): synchronous,
        between frames; pixels, accumulation and reservoirs are untouched. The host scene keeps its own tree. quality: "morton", the plain
        Morton-order tree, or "sah", the tree refined by surface area (frt_renderer_rebuild_tree_ex)."""
        if quality == "morton":
            check(lib().frt_renderer_rebuild_tree(self._h))
        else:
            check(lib().frt_renderer_rebuild_tree_ex(self._h, rebuild_mode(quality)))

    # ---- how many instances the replica holds (include/frt.h: frt_renderer_add_instances / _remove_instances): synchronous, between
    # frames, ending in the device tree rebuild `quality` names; accumulation, reservoirs and frame_count are kept. The host scene is not changed
    # (SceneBuilder has the same two methods).
    def add_instances(self, mesh_ids, mat_ids, transforms_colmajor, quality="sah"):
        """Append instances of existing meshes and materials to this renderer's scene replica; returns the id of the first new instance."""
        n, me, ma, m = instance_add_args(mesh_ids, mat_ids, transforms_colmajor)
        return check(lib().frt_renderer_add_instances(self._h, n, me.ctypes.data, ma.ctypes.data, m.ctypes.data, rebuild_mode(quality)))

    def remove_instances(self, ids, quality="sah"):
        """Remove instances from this renderer's scene replica (an id given twice once); the ids above them shift down."""
        n, i = instance_id_args(ids)
        check(lib().frt_renderer_remove_instances(self._h, n, i.ctypes.data, rebuild_mode(quality)))

    def scene_counts(self):
        """Triangles, instances, materials and lights of the replica as it is now."""
        c = (C.c_uint32 * 4)()
        check(lib().frt_renderer_scene_counts(self._h, c))
        return dict(zip(("tris", "instances", "materials", "lights"), (int(v) for v in c)))

    def pool_counts(self):
        """Meshes, vertices, indices and texture layers of the replica as it is now, and the add_* / register_* calls that had to grow a capacity."""
        c = (C.c_uint32 * 6)()
        check(lib().frt_renderer_pool_counts(self._h, c))
        return dict(zip(("meshes", "vertices", "indices", "color_layers", "data_layers", "growths"), (int(v) for v in c)))

    def add_gltf(self, model, transform_colmajor, quality="sah"):
        """Import a loaded model (frt.loader.load_gltf) into the running renderer, as SceneBuilder.add_gltf_materials / _meshes / _instances import it
        into a scene: its images become texture layers, its materials (slots remapped to those layers by the library's own remapping) and its meshes
        are appended, and one instance per primitive is added under `transform_colmajor`. Returns (mesh ids, material ids, id of the first instance)."""
        pc = self.pool_counts()
        mats, color_images, data_images = gltf_layer_plan(model, pc["color_layers"], pc["data_layers"])
        for img in color_images:
            self.add_texture(0, model.image(img))
        for img in data_images:
            self.add_texture(1, model.image(img))
        n = model.counts()["geometries"]
        geos = [model.geometry(i) for i in range(n)]
        mat0 = self.add_materials(mats)
        mat_ids = np.arange(mat0, mat0 + len(mats), dtype=np.uint32)
        mesh0 = self.add_meshes([g for g, _ in geos])
        mesh_ids = np.arange(mesh0, mesh0 + n, dtype=np.uint32)
        use = [int(mat_ids[mi]) if mi < len(mat_ids) else 0 for _, mi in geos]      # (builder.rs:294-307: a primitive without a known material uses material 0)
        m = np.tile(np.ascontiguousarray(transform_colmajor, np.float32).reshape(1, 16), (n, 1))
        return mesh_ids, mat_ids, self.add_instances(mesh_ids, use, m, quality=quality)

    def rebuild_stats(self):
        """The last rebuild_tree that reached the device: mode asked for, clustering iterations ("sah"), why the Morton tree was built instead
        (0 it was not, 1 iteration bound, 2 traversal stack), KiB of device memory the refined mode has added."""
        s = (C.c_uint32 * 4)()
        check(lib().frt_renderer_rebuild_stats(self._h, s))
        return {"mode": int(s[0]), "iterations": int(s[1]), "fell_back": int(s[2]), "refined_scratch_kib": int(s[3])}

    def tree_stats(self):
        """The replica's quad tree: nodes, traversal-stack need, levels, origin (0 host build, 1 device Morton tree, 2 device refined tree)."""
        s = (C.c_uint32 * 4)()
        check(lib().frt_renderer_tree_stats(self._h, s))
        return {"quad_nodes": int(s[0]), "quad_stack_need": int(s[1]), "quad_levels": int(s[2]), "origin": int(s[3])}

    def read_scene(self, what):
        """The device replica in SceneBuilder.get's layout: "materials", "lights", "attributes", "indices", "mesh_infos", "quad_nodes", "tri_slots", "pair_nodes",
        "instances_dev", "shade_tris"; and "normals", the decoded normal of every vertex ([vertices, 4]: xyz, 0). Syncs first."""
        n = self.scene_counts()      # (the replica's own counts: after add_instances / remove_instances they differ from the host scene's)
        if what in ("attributes", "indices", "mesh_infos", "normals"):
            p = self.pool_counts()
            which, shape, dt = {"attributes": (4, (p["vertices"], 8), np.float32), "indices": (5, (p["indices"],), np.uint32), "mesh_infos": (6, (p["meshes"], 4), np.uint32),
                                "normals": (18, (p["vertices"], 4), np.float32)}[what]
            out = np.zeros(shape, dt)
            check(lib().frt_renderer_read_scene(self._h, which, out.ctypes.data))
            return out
        which, shape, dt = {"materials": (2, (n["materials"], 16), np.uint32), "lights": (3, (n["lights"], 16), np.uint32), "quad_nodes": (10, (self.tree_stats()["quad_nodes"], 32), np.float32),
                            "tri_slots": (13, (n["tris"], 12), np.float32), "pair_nodes": (15, (self._scene.bvh_stats()["pair_nodes"], 16), np.float32),
                            "instances_dev": (16, (n["instances"], 16), np.uint32), "shade_tris": (17, (n["tris"], 32), np.float32)}[what]
        out = np.zeros(shape, dt)
        check(lib().frt_renderer_read_scene(self._h, which, out.ctypes.data))
        return out

    def stats(self):
        s = Stats()
        check(lib().frt_renderer_stats(self._h, C.byref(s)))
        return {"rays_closest": s.rays_closest, "rays_any": s.rays_any, "frames": s.frames,
                "ms_stage": list(s.ms_stage), "launches": list(s.launches),
                "rays_stage": [[int(s.rays_stage[i][0]), int(s.rays_stage[i][1])] for i in range(4)], "halo_overflow": int(s.halo_overflow),
                "ms_merge": s.ms_merge, "queue_overflow": int(s.queue_overflow), "queue_capacity": int(s.queue_capacity), "queue_bytes": int(s.queue_bytes),
                "speculated_frames": int(s.speculated_frames), "discarded_speculations": int(s.discarded_speculations)}


def _stats_dict(s):
    return {"rays_closest": s.rays_closest, "rays_any": s.rays_any, "frames": s.frames,
            "ms_stage": list(s.ms_stage), "launches": list(s.launches),
            "rays_stage": [[int(s.rays_stage[i][0]), int(s.rays_stage[i][1])] for i in range(4)], "halo_overflow": int(s.halo_overflow),
            "ms_merge": s.ms_merge, "queue_overflow": int(s.queue_overflow), "queue_capacity": int(s.queue_capacity), "queue_bytes": int(s.queue_bytes),
            "speculated_frames": int(s.speculated_frames), "discarded_speculations": int(s.discarded_speculations)}


class MultiRenderer(_HostQueries, _SceneGrowth):
    """Renderer::new / render (renderer.rs:206, :349) for several GPUs of one node through frt_multi_renderer_*: ONE process, one call per
    frame; strips, halo copies and the gather are inside libfrt.so. `devices`: HIP ordinals, repeats allowed (several strips on one GPU)."""
    _trace_closest, _trace_any, _pick = "frt_multi_renderer_trace_closest", "frt_multi_renderer_trace_any", "frt_multi_renderer_pick"
    _grow = "frt_multi_renderer_"

    def __init__(self, scene, width, height, devices, max_depth=8, motion_halo=0, flags=0, queue_capacity=0):
        o = RenderOpts()
        o.max_depth, o.flags, o.motion_halo_rows, o.queue_capacity = max_depth, flags, motion_halo, queue_capacity
        dev = (C.c_int32 * len(devices))(*devices)
        self.width, self.height, self.ndev = width, height, len(devices)
        self._scene = scene
        self._destroy = lib().frt_multi_renderer_destroy
        self._h = lib().frt_multi_renderer_create(scene._h, width, height, len(devices), dev, C.byref(o))
        if not self._h:
            raise FrtError("multi renderer creation failed: " + lib().frt_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    @property
    def frame_count(self):
        return int(lib().frt_multi_renderer_frame_count(self._h))

    def render(self, camera_uniform):
        check(lib().frt_multi_renderer_render(self._h, C.byref(camera_uniform)))

    def sync(self):
        check(lib().frt_multi_renderer_sync(self._h))

    def reset(self):
        check(lib().frt_multi_renderer_reset(self._h))

    def clear(self):
        """Back to the state right after creation on every strip; the way out of the failed state (a strip's step failed mid-frame)."""
        check(lib().frt_multi_renderer_clear(self._h))

    def set_jitter(self, jitter):
        check(lib().frt_multi_renderer_set_jitter(self._h, float(jitter[0]), float(jitter[1])))

    def inject_failure(self, strip, step):
        """Testing: the next render call fails on `strip` in step 0 (T-merge half) or 1 (spatial + post half)."""
        check(lib().frt_multi_renderer_inject_failure(self._h, strip, step))

    def peer_access(self):
        out = (C.c_uint32 * 2)()
        check(lib().frt_multi_renderer_peer_access(self._h, out))
        return {"neighbour_pairs_on_different_devices": int(out[0]), "pairs_with_peer_access": int(out[1])}

    def gather(self, buf, index, device, dst_ptr, stream=None):
        """Device-side gather of every strip's rows of `buf`[index] into the full-frame device buffer at `dst_ptr` on HIP device `device`."""
        check(lib().frt_multi_renderer_gather(self._h, buf, index, device, C.c_void_p(dst_ptr), C.c_void_p(stream) if stream else None))

    def boundaries(self):
        out = (C.c_uint32 * (self.ndev + 1))()
        check(lib().frt_multi_renderer_boundaries(self._h, out))
        return list(out)

    def set_instance_transforms(self, ids, transforms_colmajor):
        """Renderer.set_instance_transforms on every strip's scene replica. Host arrays only: the strips' replicas live on different devices."""
        if any(_is_device_tensor(x) for x in (ids, transforms_colmajor)):
            raise FrtError("set_instance_transforms: a MultiRenderer takes host arrays only (its replicas live on different devices)")
        n, i, m = transform_args(ids, transforms_colmajor)
        check(lib().frt_multi_renderer_set_instance_transforms(self._h, n, i.ctypes.data, m.ctypes.data))

    def set_mesh_vertices(self, mesh_id, positions, attributes=None, normals="keep"):
        """Renderer.set_mesh_vertices on every strip's scene replica. Host arrays only: the strips' replicas live on different devices."""
        if any(_is_device_tensor(x) for x in (positions, attributes)):
            raise FrtError("set_mesh_vertices: a MultiRenderer takes host arrays only (its replicas live on different devices)")
        set_mesh_vertices_call("frt_multi_renderer_set_mesh_vertices", self._h, mesh_id, positions, attributes, normals)

    def set_mesh_skin(self, mesh_id, joints, weights=None, num_joints=None, mode="linear"):
        """Renderer.set_mesh_skin on every strip's scene replica."""
        set_mesh_skin_call("frt_multi_renderer_set_mesh_skin", self._h, mesh_id, joints, weights, _num_joints(joints, num_joints), mode)

    def set_mesh_pose(self, mesh_id, joint_matrices, normals="recompute", morph_weights=None):
        """Renderer.set_mesh_pose on every strip's scene replica. Host arrays only: the strips' replicas live on different devices."""
        if _is_device_tensor(joint_matrices) or _is_device_tensor(morph_weights):
            raise FrtError("set_mesh_pose: a MultiRenderer takes host arrays only (its replicas live on different devices)")
        set_mesh_pose_call("frt_multi_renderer_set_mesh_pose", self._h, mesh_id, joint_matrices, normals, morph_weights)

    def set_mesh_poses(self, mesh_ids, joint_matrices=None, morph_weights=None, normals="recompute"):
        """Renderer.set_mesh_poses on every strip's scene replica. Host arrays only: the strips' replicas live on different devices."""
        if _is_device_tensor(joint_matrices) or _is_device_tensor(morph_weights):
            raise FrtError("set_mesh_poses: a MultiRenderer takes host arrays only (its replicas live on different devices)")
        set_mesh_poses_call("frt_multi_renderer_set_mesh_poses", self._h, mesh_ids, joint_matrices, morph_weights, normals)

    def animate(self, rig, mesh_ids, clip, t, normals="recompute"):
        """`rig` (frt.Rig) evaluated on the host at clip `clip`, time `t`, then set_mesh_poses on every strip's replica (host arrays, as everywhere here)."""
        self.set_mesh_poses(mesh_ids, *rig.evaluate(clip, t), normals=normals)

    def animate_instances(self, rig, instance_ids, nodes, clip, t, root=None, offsets=None):
        """rig.evaluate_nodes on the host, then set_instance_transforms on every strip's replica."""
        self.set_instance_transforms(instance_ids, rig.evaluate_nodes(clip, t, nodes, root, offsets))

    def animate_cast(self, entries, normals="recompute"):
        """The host form of Renderer.animate_cast (frt.animation.host_cast): the instance entries through animate_instances, then the mesh entries
        through animate, on every strip's replica."""
        from .animation import host_cast
        host_cast(self, entries, normals)

    def animate_blend(self, rig, mesh_ids, samples, normals="recompute"):
        """rig.evaluate_blend(samples) on the host, then set_mesh_poses on every strip's replica ("Blending clips")."""
        self.set_mesh_poses(mesh_ids, *rig.evaluate_blend(samples), normals=normals)

    def animate_instances_blend(self, rig, instance_ids, nodes, samples, root=None, offsets=None):
        """rig.evaluate_nodes_blend on the host, then set_instance_transforms on every strip's replica."""
        self.set_instance_transforms(instance_ids, rig.evaluate_nodes_blend(samples, nodes, root, offsets))

    def animate_cast_blend(self, entries, normals="recompute"):
        """The host form of Renderer.animate_cast_blend (frt.animation.host_cast_blend) on every strip's replica."""
        from .animation import host_cast_blend
        host_cast_blend(self, entries, normals)

    def animate_layers(self, rig, mesh_ids, layers, masks=None, normals="recompute", goals=None, targets=None):
        """rig.evaluate_layers(layers, masks, goals, targets) on the host, then set_mesh_poses on every strip's replica (DESIGN.md section 11,
        "Layering clips", "Inverse kinematics", "Chain IK": frt.Chain goals are solved on the host here). The targets are host arrays."""
        self.set_mesh_poses(mesh_ids, *rig.evaluate_layers(layers, masks, goals, targets), normals=normals)

    def animate_instances_layers(self, rig, instance_ids, nodes, layers, masks=None, root=None, offsets=None, goals=None, targets=None):
        """rig.evaluate_nodes_layers on the host, then set_instance_transforms on every strip's replica."""
        self.set_instance_transforms(instance_ids, rig.evaluate_nodes_layers(layers, nodes, root, offsets, masks, goals, targets))

    def animate_cast_layers(self, entries, normals="recompute"):
        """The host form of Renderer.animate_cast_layers (frt.animation.host_cast_layers) on every strip's replica."""
        from .animation import host_cast_layers
        host_cast_layers(self, entries, normals)

    def set_mesh_morph_targets(self, mesh_id, deltas):
        """Renderer.set_mesh_morph_targets on every strip's scene replica."""
        set_mesh_morph_targets_call("frt_multi_renderer_set_mesh_morph_targets", self._h, mesh_id, deltas)

    def set_mesh_morph_weights(self, mesh_id, weights, normals="recompute"):
        """Renderer.set_mesh_morph_weights on every strip's scene replica. Host arrays only: the strips' replicas live on different devices."""
        if _is_device_tensor(weights):
            raise FrtError("set_mesh_morph_weights: a MultiRenderer takes host arrays only (its replicas live on different devices)")
        set_mesh_morph_weights_call("frt_multi_renderer_set_mesh_morph_weights", self._h, mesh_id, weights, normals)

    # ---- what the replica looks like (include/frt.h: frt_renderer_set_materials and the three calls after it): asynchronous,
    # between frames, the arguments copied during the call; accumulation and reservoirs are kept (reset() / clear() to converge to the new look).
    # The host scene is not changed (SceneBuilder has the same four methods).
    def set_materials(self, ids, materials):
        """Material ids[k] of every strip's scene replica becomes materials[k]."""
        n, i, m = material_args(ids, materials)
        check(lib().frt_multi_renderer_set_materials(self._h, n, i.ctypes.data, m.ctypes.data))

    def set_instance_materials(self, instance_ids, material_ids):
        """Instance instance_ids[k] uses material material_ids[k]; pick and trace_closest report it at once."""
        n, i, m = id_pair_args(instance_ids, material_ids)
        check(lib().frt_multi_renderer_set_instance_materials(self._h, n, i.ctypes.data, m.ctypes.data))

    def set_light_emission(self, light, color, intensity):
        """Light `light` emits (color, intensity); a light registered with an instance also gets that instance's emissive material updated."""
        l, c, i = emission_args(light, color, intensity)
        check(lib().frt_multi_renderer_set_light_emission(self._h, l, c.ctypes.data, i))

    def set_texture(self, kind, layer, rgba8):
        """Replace one existing texture layer: kind "color" (0) or "data" (1), rgba8 1024 x 1024 x 4 bytes."""
        k, l, t = texture_args(kind, layer, rgba8)
        check(lib().frt_multi_renderer_set_texture(self._h, k, l, t.ctypes.data))

    def trace_closest(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        """Renderer.trace_closest on the first strip's replica (all are equal); host arrays only."""
        return self._host_trace_closest(origins, dirs, tmin, tmax)

    def trace_any(self, origins, dirs, tmin=0.0, tmax=3.0e38):
        return self._host_trace_any(origins, dirs, tmin, tmax)

    def pick(self, camera_uniform, xy):
        """Renderer.pick in the full frame, on the first strip's replica; host arrays only."""
        return self._host_pick(camera_uniform, xy)

    def rebuild_tree(self, quality="morton"):
        """Renderer.rebuild_tree on every strip's scene replica."""
        if quality == "morton":
            check(lib().frt_multi_renderer_rebuild_tree(self._h))
        else:
            check(lib().frt_multi_renderer_rebuild_tree_ex(self._h, rebuild_mode(quality)))

    def add_instances(self, mesh_ids, mat_ids, transforms_colmajor, quality="sah"):
        """Renderer.add_instances on every strip's scene replica."""
        n, me, ma, m = instance_add_args(mesh_ids, mat_ids, transforms_colmajor)
        return check(lib().frt_multi_renderer_add_instances(self._h, n, me.ctypes.data, ma.ctypes.data, m.ctypes.data, rebuild_mode(quality)))

    def remove_instances(self, ids, quality="sah"):
        """Renderer.remove_instances on every strip's scene replica."""
        n, i = instance_id_args(ids)
        check(lib().frt_multi_renderer_remove_instances(self._h, n, i.ctypes.data, rebuild_mode(quality)))

    def read_buffer(self, buf, index=0):
        out = np.zeros((self.height, self.width, BUF_BPP[buf]), np.uint8)
        check(lib().frt_multi_renderer_read_buffer(self._h, buf, index, out.ctypes.data))
        return out

    def read_display(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        check(lib().frt_multi_renderer_read_display(self._h, out.ctypes.data))
        return out

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(lib().frt_multi_renderer_read_accum(self._h, out.ctypes.data))
        return out

    def stats(self):
        s = Stats()
        check(lib().frt_multi_renderer_stats(self._h, C.byref(s)))
        return _stats_dict(s)
