"""Every route through the staging of the mesh-edit family on one renderer (include/frt.h: frt_renderer_set_mesh_vertices_ex, _set_mesh_pose,
_set_mesh_pose_ex, _set_mesh_morph_weights): host positions with and without attributes and recomputed normals, device
positions, host and device palettes, host and device weights, alone and together, alternating between a 4-vertex and an 8-vertex mesh, so that every
section of the call's pinned and device blocks is empty in some call and filled in another and the blocks shrink and regrow. After each call the replica
equals the host scene bit for bit; a NaN weight on the device is counted and changes nothing; the last frames equal the brute-force oracle's.
The second part holds the renderer's and the multi renderer's order of refusals: the rows of tests/_mesh_calls.py and rows with device pointers, each
wrong in two ways, with the code and the message recorded before the family's checks were gathered."""
import ctypes as C
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_normals_gpu import check_replica, REPLICA
from test_mesh_skin_gpu import torch_dev, _up      # noqa: F401  (torch_dev: a fixture)
from _mesh_calls import F, QUAD, STRIP, SPARE, NVERTS, REC, DEV, BAD, pose_scene, pose_meshes, refusal_rows, bind_for_refusals, run_row
from _skin_model import make_skin, make_palette, skin_model
from _morph_model import make_targets, make_weights, morph_model

pytestmark = pytest.mark.gpu
W = H = 16
EVERY = REPLICA + ("normals",)


def _bent(g, phase):
    """The mesh's positions moved a little, and attributes with shifted uvs (same topology, same normals)."""
    p = np.array(g.positions, F)
    p[:, 1] += F(0.05) * np.sin(F(3.0) * p[:, 0] + F(phase)).astype(F)
    a = np.array(g.attributes, F)
    a[:, 2:4] += F(0.125) * F(phase)
    return p, a


def _routes(meshes):
    """[(what, mesh, method, host arguments, which of them go up as device tensors, keywords)], the meshes alternating."""
    out = []
    k = 0

    def add(what, m, method, args, dev=(), **kw):
        out.append((f"{len(out)}: {what}, mesh {m}", m, method, args, dev, kw))

    for m in (QUAD, STRIP):
        p, a = _bent(meshes[m], 0.3 + m)
        add("host positions", m, "set_mesh_vertices", (p,))
    for m in (STRIP, QUAD):
        p, a = _bent(meshes[m], 0.7 + m)
        add("host positions and attributes", m, "set_mesh_vertices", (p, a))
    for m in (QUAD, STRIP):
        p, a = _bent(meshes[m], 1.1 + m)
        add("host positions, recompute", m, "set_mesh_vertices", (p,), normals="recompute")
    p, a = _bent(meshes[STRIP], 1.3)
    add("host positions and attributes, recompute", STRIP, "set_mesh_vertices", (p, a), normals="recompute")
    for m, with_attrs in ((QUAD, False), (STRIP, True), (STRIP, False), (QUAD, True)):
        p, a = _bent(meshes[m], 1.5 + m)
        add("device positions" + (" and attributes" if with_attrs else ""), m, "set_mesh_vertices", (p, a) if with_attrs else (p,), dev=(0, 1) if with_attrs else (0,))
    p, a = _bent(meshes[QUAD], 1.9)
    add("device positions, recompute", QUAD, "set_mesh_vertices", (p,), dev=(0,), normals="recompute")
    for normals in ("keep", "recompute"):
        for k, (what, dev) in enumerate((("host", False), ("device", True))):
            m, o = (QUAD, STRIP)[k], (STRIP, QUAD)[k]
            ph = 0.2 + 0.4 * k + (0.1 if normals == "keep" else 0.0)
            add(f"pose, {what} palette, {normals}", m, "set_mesh_pose", (make_palette(2, ph),), dev=(0,) if dev else (), normals=normals)
            add(f"morph, {what} weights, {normals}", o, "set_mesh_morph_weights", (make_weights(2, ph),), dev=(0,) if dev else (), normals=normals)
            add(f"pose and morph, {what} inputs, {normals}", o, "set_mesh_pose", (make_palette(2, ph + 1.0),), dev=(0, "morph_weights") if dev else (),
                normals=normals, morph_weights=make_weights(2, ph + 1.0))
            add(f"pose and morph, {what} inputs, {normals}", m, "set_mesh_pose", (make_palette(2, ph + 2.0),), dev=(0, "morph_weights") if dev else (),
                normals=normals, morph_weights=make_weights(2, ph + 2.0))
    return out


def test_every_route_equals_the_host_scene(gpu, orc, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs, meshes = pose_scene(frt)
    r = frt.Renderer(fs, W, H, max_depth=4)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    skins = {m: make_skin(NVERTS[m], 2, seed=m) for m in (QUAD, STRIP, SPARE)}
    targets = {m: make_targets(NVERTS[m], 2, seed=m) for m in (QUAD, STRIP, SPARE)}
    for x in (r, fs):
        for m in (QUAD, STRIP, SPARE):
            x.set_mesh_skin(m, *skins[m], num_joints=2)
            x.set_mesh_morph_targets(m, targets[m])
    check_replica(frt, r, fs, "after the bind calls")
    routes = _routes(meshes)
    seen = set()
    for what, m, method, args, on_dev, kw in routes:
        seen.add((method, bool(on_dev), len(args), "morph_weights" in kw, kw.get("normals", "keep")))
        rargs = [_up(torch, dev, a) if k in on_dev else a for k, a in enumerate(args)]
        rkw = {k: (_up(torch, dev, v) if k in on_dev else v) for k, v in kw.items()}
        getattr(r, method)(m, *rargs, **rkw)
        getattr(fs, method)(m, *args, **kw)
        check_replica(frt, r, fs, what)
    assert len(seen) >= 19 and r.deform_rejects() == 0
    # a host route on the mesh no instance uses: no triangle changes, its attributes do
    slots = r.read_scene("tri_slots").tobytes()
    p, a = _bent(meshes[SPARE], 0.9)
    for x in (r, fs):
        x.set_mesh_vertices(SPARE, p, a, normals="recompute")
        x.set_mesh_pose(SPARE, make_palette(2, 0.4), morph_weights=make_weights(2, 0.4))
    check_replica(frt, r, fs, "the mesh without an instance")
    assert r.read_scene("tri_slots").tobytes() == slots
    # one NaN weight from the device: counted, nothing applied
    before = {w: r.read_scene(w).tobytes() for w in EVERY}
    bad = make_weights(2, 0.5); bad[1] = np.nan
    r.set_mesh_morph_weights(STRIP, _up(torch, dev, bad))
    assert r.deform_rejects() == 1
    assert {w: r.read_scene(w).tobytes() for w in EVERY} == before
    check_replica(frt, r, fs, "after the rejected call")
    # the last frames against the oracle over a scene built from scratch: the last call of either mesh was the combined one with host... device inputs
    last = {m: [x for x in routes if x[1] == m][-1] for m in (QUAD, STRIP)}
    final = list(pose_meshes(frt))
    for m, (_, _, method, args, _, kw) in last.items():
        assert method == "set_mesh_pose" and "morph_weights" in kw
        pos = skin_model(morph_model(meshes[m].positions, targets[m], kw["morph_weights"]), *skins[m], args[0])
        mi = fs.get("mesh_infos")[m]
        final[m] = frt.geometry.Geometry(pos, fs.get("attributes")[mi[0]:mi[0] + len(pos)].copy(), meshes[m].indices)
    oh = orc.L.orc_scene_create()
    for g in final:
        pos, att, idx = (np.ascontiguousarray(v, t) for v, t in ((g.positions, F), (g.attributes, F), (g.indices, np.uint32)))
        orc.L.orc_scene_add_mesh(oh, pos.ctypes.data, pos.shape[0], att.ctypes.data, idx.ctypes.data, idx.size)
    for row in fs.get("materials"):
        orc.L.orc_scene_add_material(oh, np.ascontiguousarray(row).ctypes.data)
    for row in fs.get("lights"):
        orc.L.orc_scene_add_light(oh, np.ascontiguousarray(row).ctypes.data)
    for row in fs.get("instances"):
        orc.L.orc_scene_add_instance(oh, int(row[0]), int(row[1]), np.ascontiguousarray(row[5:21]).ctypes.data)
    orc.L.orc_scene_build(oh)
    from _oracle import OrcScene
    osc = OrcScene(orc, oh)
    assert osc.get("tris").tobytes() == fs.get("tris").tobytes()      # the numpy model's positions are the host scene's
    ro = osc.renderer(W, H, 4, False, 4)                              # brute force: nothing of the product feeds it
    r.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        r.render(cam); ro.render(cam)
        compare_all(r.read_buffer, ro.read, f, "after every route, against the oracle")
    st, so = r.stats(), ro.stats()["total"]
    assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"]) and st["rays_closest"] > 0


# ------------------------------------------------------------------------------------------------ the order of refusals
class _Short:
    """A device allocation of its own, `n` bytes (torch's allocator hands out pieces of larger ones, which no call could find too short)."""

    def __init__(self, frt, n):
        self.L, self.p = frt.lib(), C.c_void_p()
        self.L.hipMalloc.argtypes, self.L.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        self.L.hipFree.argtypes, self.L.hipFree.restype = [C.c_void_p], C.c_int
        assert self.L.hipMalloc(C.byref(self.p), n) == 0

    def free(self):
        if self.p:
            self.L.hipFree(self.p); self.p = C.c_void_p()


def device_rows(frt, torch, dev, short):
    """[(row id, call, args)]: calls with FRT_DEFORM_DEVICE that are wrong in two ways; an int argument in a pointer's place is a device address."""
    g = pose_meshes(frt)[QUAD]
    pos, att = _up(torch, dev, g.positions), _up(torch, dev, g.attributes)
    pal, wt, wt3 = _up(torch, dev, make_palette(2)), _up(torch, dev, make_weights(2)), _up(torch, dev, make_weights(3))
    hpos, hwt = np.array(g.positions, F), make_weights(2)
    s = short.p.value
    rows = [
        ("device vertices: misaligned positions, short attributes", "set_mesh_vertices_ex", (QUAD, pos.data_ptr() + 4, s, 4, DEV)),
        ("device vertices: short positions, misaligned attributes", "set_mesh_vertices_ex", (QUAD, s, att.data_ptr() + 4, 4, DEV | REC)),
        ("device vertices: wrong count, host positions", "set_mesh_vertices_ex", (QUAD, hpos, None, 5, DEV)),
        ("device vertices: null positions, wrong count", "set_mesh_vertices_ex", (QUAD, None, s, 5, DEV)),
        ("device vertices: host positions, misaligned attributes", "set_mesh_vertices_ex", (QUAD, hpos, att.data_ptr() + 4, 4, DEV)),
        ("device vertices: bad id, misaligned positions", "set_mesh_vertices_ex", (BAD, pos.data_ptr() + 4, None, 4, DEV)),
        ("device pose: no skin, misaligned palette", "set_mesh_pose", (STRIP, pal.data_ptr() + 4, 2, DEV)),
        ("device pose: wrong count, short palette", "set_mesh_pose", (QUAD, s, 3, DEV | REC)),
        ("device pose: short palette, recompute", "set_mesh_pose", (QUAD, s, 2, DEV | REC)),
        ("device pose_ex: misaligned palette, wrong weight count", "set_mesh_pose_ex", (QUAD, pal.data_ptr() + 4, 2, wt3.data_ptr(), 3, DEV)),
        ("device pose_ex: short palette, host weights", "set_mesh_pose_ex", (QUAD, s, 2, hwt, 2, DEV)),
        ("device pose_ex: wrong weight count, misaligned weights", "set_mesh_pose_ex", (QUAD, pal.data_ptr(), 2, wt3.data_ptr() + 2, 3, DEV)),
        ("device pose_ex: misaligned weights, recompute", "set_mesh_pose_ex", (QUAD, pal.data_ptr(), 2, wt.data_ptr() + 2, 2, DEV | REC)),
        ("device pose_ex: no skin, no targets, misaligned both", "set_mesh_pose_ex", (STRIP, pal.data_ptr() + 4, 2, wt.data_ptr() + 2, 2, DEV)),
        ("device weights: wrong count, misaligned weights", "set_mesh_morph_weights", (QUAD, wt3.data_ptr() + 2, 3, DEV | REC)),
        ("device weights: no targets, host weights", "set_mesh_morph_weights", (STRIP, hwt, 2, DEV)),
        ("device weights: short weights", "set_mesh_morph_weights", (QUAD, s + 44, 2, DEV)),
        ("device weights: host weights", "set_mesh_morph_weights", (QUAD, hwt, 2, DEV | REC)),
    ]
    return rows, (pos, att, pal, wt, wt3)


def python_rows(frt, torch, dev, r, multi):
    """[(row id, callable)]: the Python layer's own refusals, each call wrong in two ways."""
    g = pose_meshes(frt)[QUAD]
    pos, att = _up(torch, dev, g.positions), _up(torch, dev, g.attributes)
    pal, wt = _up(torch, dev, make_palette(2)), _up(torch, dev, make_weights(2))
    hpal, hwt = make_palette(2), make_weights(2)
    return [
        ("python vertices: mixed inputs, bad id", lambda: r.set_mesh_vertices(BAD, pos, np.array(g.attributes, F))),
        ("python vertices: mixed inputs, bad normals", lambda: r.set_mesh_vertices(QUAD, np.array(g.positions, F), att, normals="smooth")),
        ("python vertices: bad normals, negative id", lambda: r.set_mesh_vertices(-1, pos, att, normals="smooth")),
        ("python vertices: negative id, wrong dtype", lambda: r.set_mesh_vertices(-1, pos.double(), att)),
        ("python vertices: wrong dtype, attribute count", lambda: r.set_mesh_vertices(QUAD, pos.double(), att[:3].contiguous())),
        ("python vertices: wrong attribute shape and count", lambda: r.set_mesh_vertices(QUAD, pos, att[:3, :4].contiguous())),
        ("python vertices: attribute count, bad id", lambda: r.set_mesh_vertices(BAD, pos, att[:3].contiguous())),
        ("python pose: mixed inputs, bad normals", lambda: r.set_mesh_pose(QUAD, pal, normals="smooth", morph_weights=hwt)),
        ("python pose: mixed inputs the other way, bad id", lambda: r.set_mesh_pose(BAD, hpal, morph_weights=wt)),
        ("python pose: bad normals, negative id", lambda: r.set_mesh_pose(-1, pal, normals="smooth")),
        ("python pose: negative id, flat palette", lambda: r.set_mesh_pose(-1, pal.reshape(-1))),
        ("python pose: flat palette, wrong weight dtype", lambda: r.set_mesh_pose(QUAD, pal.reshape(-1), morph_weights=wt.double())),
        ("python pose: wrong weight dtype, bad id", lambda: r.set_mesh_pose(BAD, pal, morph_weights=wt.double())),
        ("python weights: bad normals, negative id", lambda: r.set_mesh_morph_weights(-1, wt, normals="smooth")),
        ("python weights: negative id, wrong shape", lambda: r.set_mesh_morph_weights(-1, wt.reshape(2, 1))),
        ("python weights: wrong shape, bad id", lambda: r.set_mesh_morph_weights(BAD, wt.reshape(2, 1))),
        ("python multi vertices: a tensor, bad id", lambda: multi.set_mesh_vertices(BAD, pos)),
        ("python multi pose: tensor weights, bad normals", lambda: multi.set_mesh_pose(QUAD, hpal, normals="smooth", morph_weights=wt)),
        ("python multi weights: a tensor, bad normals", lambda: multi.set_mesh_morph_weights(QUAD, wt, normals="smooth")),
    ]


def run_python_row(fn):
    try:
        fn()
    except Exception as e:      # noqa: BLE001  (the row records whatever type is raised)
        return type(e).__name__, str(e)
    return "no exception", ""


EXPECT_RENDERER = {
    'vertices: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'vertices: null positions, wrong count':
        (-1, 'set_mesh_vertices: null positions'),
    'vertices: NaN position, NaN attributes':
        (-1, 'set_mesh_vertices: position of vertex 3 is not finite'),
    'vertices_ex: device flag, unknown bit':
        (-1, 'set_mesh_vertices: unknown flag bits'),
    'vertices_ex: unknown bit, bad id':
        (-1, 'set_mesh_vertices: unknown flag bits'),
    'vertices_ex: device flag, bad id':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices_ex: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices_ex: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'skin: bad id, null joints':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: bad id, null weights':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: null weights, wrong count':
        (-1, 'set_mesh_skin: null joints or weights'),
    'skin: wrong count, NaN weight':
        (-1, 'set_mesh_skin: 5 vertices given, the mesh has 4'),
    'skin: no joints, a joint out of range':
        (-1, 'set_mesh_skin: 0 joints (1 to 65536: a joint index is 16 bits)'),
    'skin: a joint out of range, a negative weight':
        (-1, 'set_mesh_skin: vertex 0 names joint 1 of 1'),
    'pose: device flag, unknown bit':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose: device flag, bad id':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose: bad id, null palette':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose: wrong count, NaN entry':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: wrong count, null palette':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: no skin, wrong count':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose: no skin, null palette':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: device flag, unknown bit':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: unknown bit, bad id, no weights':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: bad id, null palette, null weights':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose_ex: no skin, no targets':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: no skin, wrong count, no weights':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: NaN palette, NaN weight':
        (-1, 'set_mesh_pose: joint matrix 0 has a non-finite entry'),
    'pose_ex: wrong palette count, wrong weight count':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose_ex: null palette, null weights':
        (-1, 'set_mesh_pose: null joint matrices'),
    'pose_ex: wrong weight count, NaN weight':
        (-1, 'set_mesh_pose: 3 weights given, 2 targets are bound'),
    'pose_ex: null weights with a count':
        (-1, 'set_mesh_pose: null weights'),
    'pose_ex: weights with no count':
        (-1, 'set_mesh_pose: 0 weights given, 2 targets are bound'),
    'targets: bad id, null deltas':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: bad id, no targets':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: wrong count, NaN delta':
        (-1, 'set_mesh_morph_targets: 5 vertices given, the mesh has 4'),
    'targets: no targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 0 targets (1 to 4096)'),
    'targets: too many targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 4097 targets (1 to 4096)'),
    'weights: device flag, unknown bit':
        (-1, 'set_mesh_morph_weights: unknown flag bits'),
    'weights: unknown bit, bad id':
        (-1, 'set_mesh_morph_weights: unknown flag bits'),
    'weights: device flag, bad id':
        (-1, 'set_mesh_morph_weights: mesh id 99 out of range (3 meshes)'),
    'weights: bad id, null weights':
        (-1, 'set_mesh_morph_weights: mesh id 99 out of range (3 meshes)'),
    'weights: wrong count, NaN weight':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: wrong count, null weights':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: no targets, wrong count':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
    'weights: no targets, null weights':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
}
EXPECT_DEVICE = {
    'device vertices: misaligned positions, short attributes':
        (-1, 'set_mesh_vertices: positions: device pointers must be 16-byte aligned'),
    'device vertices: short positions, misaligned attributes':
        (-1, 'set_mesh_vertices: positions: the device allocation holds 48 bytes from the pointer on, 64 are needed'),
    'device vertices: wrong count, host positions':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'device vertices: null positions, wrong count':
        (-1, 'set_mesh_vertices: null positions'),
    'device vertices: host positions, misaligned attributes':
        (-1, "set_mesh_vertices: positions are not memory of the renderer's device 0 (FRT_DEFORM_DEVICE)"),
    'device vertices: bad id, misaligned positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'device pose: no skin, misaligned palette':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'device pose: wrong count, short palette':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'device pose: short palette, recompute':
        (-1, 'set_mesh_pose: joint matrices: the device allocation holds 48 bytes from the pointer on, 128 are needed'),
    'device pose_ex: misaligned palette, wrong weight count':
        (-1, 'set_mesh_pose: joint matrices: device pointers must be 16-byte aligned'),
    'device pose_ex: short palette, host weights':
        (-1, 'set_mesh_pose: joint matrices: the device allocation holds 48 bytes from the pointer on, 128 are needed'),
    'device pose_ex: wrong weight count, misaligned weights':
        (-1, 'set_mesh_pose: 3 weights given, 2 targets are bound'),
    'device pose_ex: misaligned weights, recompute':
        (-1, 'set_mesh_pose: morph weights: device pointers must be 4-byte aligned'),
    'device pose_ex: no skin, no targets, misaligned both':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'device weights: wrong count, misaligned weights':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'device weights: no targets, host weights':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
    'device weights: short weights':
        (-1, 'set_mesh_morph_weights: morph weights: the device allocation holds 4 bytes from the pointer on, 8 are needed'),
    'device weights: host weights':
        (-1, "set_mesh_morph_weights: morph weights are not memory of the renderer's device 0 (FRT_DEFORM_DEVICE)"),
}
EXPECT_MULTI = {
    'vertices: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'vertices: null positions, wrong count':
        (-1, 'set_mesh_vertices: null positions'),
    'vertices: NaN position, NaN attributes':
        (-1, 'set_mesh_vertices: position of vertex 3 is not finite'),
    'vertices_ex: device flag, unknown bit':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'vertices_ex: unknown bit, bad id':
        (-1, 'set_mesh_vertices: unknown flag bits'),
    'vertices_ex: device flag, bad id':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'vertices_ex: bad id, null positions':
        (-1, 'set_mesh_vertices: mesh id 99 out of range (3 meshes)'),
    'vertices_ex: wrong count, NaN position':
        (-1, 'set_mesh_vertices: 5 vertices given, the mesh has 4 (the topology is fixed)'),
    'skin: bad id, null joints':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: bad id, null weights':
        (-1, 'set_mesh_skin: mesh id 99 out of range (3 meshes)'),
    'skin: null weights, wrong count':
        (-1, 'set_mesh_skin: null joints or weights'),
    'skin: wrong count, NaN weight':
        (-1, 'set_mesh_skin: 5 vertices given, the mesh has 4'),
    'skin: no joints, a joint out of range':
        (-1, 'set_mesh_skin: 0 joints (1 to 65536: a joint index is 16 bits)'),
    'skin: a joint out of range, a negative weight':
        (-1, 'set_mesh_skin: vertex 0 names joint 1 of 1'),
    'pose: device flag, unknown bit':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'pose: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose: device flag, bad id':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'pose: bad id, null palette':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose: wrong count, NaN entry':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: wrong count, null palette':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose: no skin, wrong count':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose: no skin, null palette':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: device flag, unknown bit':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'pose_ex: unknown bit, bad id':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: unknown bit, bad id, no weights':
        (-1, 'set_mesh_pose: unknown flag bits'),
    'pose_ex: bad id, null palette, null weights':
        (-1, 'set_mesh_pose: mesh id 99 out of range (3 meshes)'),
    'pose_ex: no skin, no targets':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: no skin, wrong count, no weights':
        (-1, 'set_mesh_pose: the mesh has no skin (set_mesh_skin)'),
    'pose_ex: NaN palette, NaN weight':
        (-1, 'set_mesh_pose: joint matrix 0 has a non-finite entry'),
    'pose_ex: wrong palette count, wrong weight count':
        (-1, 'set_mesh_pose: 3 joint matrices given, the skin was bound with 2'),
    'pose_ex: null palette, null weights':
        (-1, 'set_mesh_pose: null joint matrices'),
    'pose_ex: wrong weight count, NaN weight':
        (-1, 'set_mesh_pose: 3 weights given, 2 targets are bound'),
    'pose_ex: null weights with a count':
        (-1, 'set_mesh_pose: null weights'),
    'pose_ex: weights with no count':
        (-1, 'set_mesh_pose: 0 weights given, 2 targets are bound'),
    'targets: bad id, null deltas':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: bad id, no targets':
        (-1, 'set_mesh_morph_targets: mesh id 99 out of range (3 meshes)'),
    'targets: wrong count, NaN delta':
        (-1, 'set_mesh_morph_targets: 5 vertices given, the mesh has 4'),
    'targets: no targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 0 targets (1 to 4096)'),
    'targets: too many targets, NaN delta':
        (-1, 'set_mesh_morph_targets: 4097 targets (1 to 4096)'),
    'weights: device flag, unknown bit':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'weights: unknown bit, bad id':
        (-1, 'set_mesh_morph_weights: unknown flag bits'),
    'weights: device flag, bad id':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'weights: bad id, null weights':
        (-1, 'set_mesh_morph_weights: mesh id 99 out of range (3 meshes)'),
    'weights: wrong count, NaN weight':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: wrong count, null weights':
        (-1, 'set_mesh_morph_weights: 3 weights given, 2 targets are bound'),
    'weights: no targets, wrong count':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
    'weights: no targets, null weights':
        (-1, 'set_mesh_morph_weights: the mesh has no morph targets (set_mesh_morph_targets)'),
    'device vertices: misaligned positions, short attributes':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device vertices: short positions, misaligned attributes':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device vertices: wrong count, host positions':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device vertices: null positions, wrong count':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device vertices: host positions, misaligned attributes':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device vertices: bad id, misaligned positions':
        (-1, "multi set_mesh_vertices: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose: no skin, misaligned palette':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose: wrong count, short palette':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose: short palette, recompute':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose_ex: misaligned palette, wrong weight count':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose_ex: short palette, host weights':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose_ex: wrong weight count, misaligned weights':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose_ex: misaligned weights, recompute':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device pose_ex: no skin, no targets, misaligned both':
        (-1, "multi set_mesh_pose: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device weights: wrong count, misaligned weights':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device weights: no targets, host weights':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device weights: short weights':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
    'device weights: host weights':
        (-1, "multi set_mesh_morph_weights: FRT_DEFORM_DEVICE is refused (the strips' replicas live on different devices)"),
}
EXPECT_PYTHON = {
    'python vertices: mixed inputs, bad id':
        ('FrtError', 'set_mesh_vertices: positions and attributes must both be host arrays or both be device tensors'),
    'python vertices: mixed inputs, bad normals':
        ('FrtError', 'set_mesh_vertices: positions and attributes must both be host arrays or both be device tensors'),
    'python vertices: bad normals, negative id':
        ('FrtError', 'set_mesh_vertices: normals must be "keep" or "recompute", not \'smooth\''),
    'python vertices: negative id, wrong dtype':
        ('FrtError', 'mesh id must be an unsigned 32-bit index'),
    'python vertices: wrong dtype, attribute count':
        ('FrtError', 'set_mesh_vertices: device positions must be a contiguous float32 tensor shaped [n, 4]'),
    'python vertices: wrong attribute shape and count':
        ('FrtError', 'set_mesh_vertices: device attributes must be a contiguous float32 tensor shaped [n, 8]'),
    'python vertices: attribute count, bad id':
        ('FrtError', '4 positions but 3 attribute records'),
    'python pose: mixed inputs, bad normals':
        ('TypeError', 'set_mesh_pose: joint matrices and morph weights must both be host arrays or both be device tensors'),
    'python pose: mixed inputs the other way, bad id':
        ('TypeError', 'set_mesh_pose: joint matrices and morph weights must both be host arrays or both be device tensors'),
    'python pose: bad normals, negative id':
        ('FrtError', 'set_mesh_vertices: normals must be "keep" or "recompute", not \'smooth\''),
    'python pose: negative id, flat palette':
        ('FrtError', 'mesh id must be an unsigned 32-bit index'),
    'python pose: flat palette, wrong weight dtype':
        ('FrtError', 'set_mesh_pose: device joint matrices must be a contiguous float32 tensor shaped [J, 16] or [J, 4, 4]'),
    'python pose: wrong weight dtype, bad id':
        ('FrtError', 'set_mesh_pose: device morph weights must be a contiguous float32 tensor shaped [T]'),
    'python weights: bad normals, negative id':
        ('FrtError', 'set_mesh_vertices: normals must be "keep" or "recompute", not \'smooth\''),
    'python weights: negative id, wrong shape':
        ('FrtError', 'mesh id must be an unsigned 32-bit index'),
    'python weights: wrong shape, bad id':
        ('FrtError', 'set_mesh_morph_weights: device morph weights must be a contiguous float32 tensor shaped [T]'),
    'python multi vertices: a tensor, bad id':
        ('FrtError', 'set_mesh_vertices: a MultiRenderer takes host arrays only (its replicas live on different devices)'),
    'python multi pose: tensor weights, bad normals':
        ('FrtError', 'set_mesh_pose: a MultiRenderer takes host arrays only (its replicas live on different devices)'),
    'python multi weights: a tensor, bad normals':
        ('FrtError', 'set_mesh_morph_weights: a MultiRenderer takes host arrays only (its replicas live on different devices)'),
}


@pytest.fixture(scope="module")
def targets_of_refusals(gpu, torch_dev):
    frt = gpu
    fs, _ = pose_scene(frt)
    r, multi = frt.Renderer(fs, W, H), frt.MultiRenderer(fs, 64, 48, [0, 0])      # (two strips of 16 x 16 would be thinner than the halo)
    for x in (r, multi):
        bind_for_refusals(x)
    short = _Short(frt, 48)
    yield r, multi, short
    multi.sync(); r.sync()
    short.free()


def collect_refusals(frt, torch, dev, r, multi, short):
    """Every row's outcome: {"renderer": {row id: (code, message)}, "device": ..., "multi": ..., "python": {row id: (exception type, text)}}."""
    drows, keep = device_rows(frt, torch, dev, short)
    out = {"renderer": {rid: run_row(frt, "frt_renderer_", r._h, c, a) for rid, c, a in refusal_rows(frt, "renderer")},
           "device": {rid: run_row(frt, "frt_renderer_", r._h, c, a) for rid, c, a in drows},
           "multi": {rid: run_row(frt, "frt_multi_renderer_", multi._h, c, a) for rid, c, a in refusal_rows(frt, "multi") + drows},
           "python": {rid: run_python_row(fn) for rid, fn in python_rows(frt, torch, dev, r, multi)}}
    del keep
    return out


def test_order_of_refusals(gpu, torch_dev, targets_of_refusals):
    frt = gpu
    torch, dev = torch_dev
    r, multi, short = targets_of_refusals
    before = {w: r.read_scene(w).tobytes() for w in EVERY}
    got = collect_refusals(frt, torch, dev, r, multi, short)
    for part, want in (("renderer", EXPECT_RENDERER), ("device", EXPECT_DEVICE), ("multi", EXPECT_MULTI), ("python", EXPECT_PYTHON)):
        assert list(got[part]) == list(want), part
        for rid in want:
            assert got[part][rid] == want[rid], f"{part}: {rid}"
    assert len(EXPECT_RENDERER) >= 48 and len(EXPECT_DEVICE) >= 18 and len(EXPECT_MULTI) >= 66 and len(EXPECT_PYTHON) >= 19
    assert r.deform_rejects() == 0 and {w: r.read_scene(w).tobytes() for w in EVERY} == before
