"""What the tests of the mesh-edit family share (include/frt.h: the seven *_set_mesh_* calls of a scene, a renderer and a multi renderer; DESIGN.md
section 11): one tiny scene whose meshes differ in size, and one table of calls that are wrong in two or more ways at once. A row names the C call
without its prefix; tests/test_mesh_call_refusals.py runs the rows against a scene, tests/test_mesh_pose_routes_gpu.py against a renderer and a multi
renderer, each with the code and the message it expects written out."""
import numpy as np

F = np.float32
QUAD, STRIP, SPARE = 0, 1, 2            # mesh ids of pose_scene: 4 vertices and two instances, 8 vertices and one instance, 6 vertices and no instance
NVERTS = {QUAD: 4, STRIP: 8, SPARE: 6}
REC, DEV, UNK = 1, 2, 4                 # FRT_DEFORM_RECOMPUTE_NORMALS, FRT_DEFORM_DEVICE, a bit no call knows
BAD = 99                                # a mesh id no scene here has


def strip(frt, nx):
    """A strip of nx x 2 vertices in the plane y = 0, x in [-0.5, 0.5], z in [-0.25, 0.25]: 2 (nx - 1) triangles, normals +y."""
    xs = np.linspace(-0.5, 0.5, nx, dtype=F)
    pos = np.array([[x, 0.0, z, 1.0] for x in xs for z in (-0.25, 0.25)], F)
    att = np.zeros((2 * nx, 8), F)
    att[:, 0:2] = frt.geometry.encode_octahedral_normal([0.0, 1.0, 0.0])
    att[:, 2] = pos[:, 0] + F(0.5); att[:, 3] = pos[:, 2] * F(2.0) + F(0.5)
    att[:, 4:8] = (1.0, 0.0, 0.0, 1.0)
    idx = []
    for k in range(nx - 1):
        a = 2 * k
        idx += [a, a + 1, a + 2, a + 2, a + 1, a + 3]
    return frt.geometry.Geometry(pos, att, np.array(idx, np.uint32))


def pose_meshes(frt):
    return [frt.geometry.create_plane(), strip(frt, 4), strip(frt, 3)]


def pose_scene(frt, build=True, meshes=None):
    """(scene, meshes): the quad as a floor and as a back wall, the 8-vertex strip once (mirrored, tilted towards the camera), the 6-vertex strip in the
    pools only; one quad light that no instance carries. `meshes`: three others in their places."""
    from frt.scenes import _T, _S, _RX, _mul
    meshes = pose_meshes(frt) if meshes is None else meshes
    b = frt.SceneBuilder()
    for g in meshes:
        b.add_mesh(g)
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    red = b.add_material(frt.material_new([0.65, 0.05, 0.05, 1.0]))
    b.add_instance(QUAD, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.add_instance(QUAD, grey, _mul(_T(0.0, 0.0, -1.5), _RX(np.pi / 2), _S(4.0)))
    b.add_instance(STRIP, red, _mul(_T(0.1, -0.3, 0.0), _RX(0.6), np.diag(np.array([-1.5, 1.5, 1.5, 1.0], F))))
    l = frt.Light()
    l.position[:] = (0.0, 1.5, 0.5); l.type_ = 0
    l.u[:] = (0.5, 0.0, 0.0); l.v[:] = (0.0, 0.0, 0.5); l.area = 1.0
    l.emission[:] = (1.0, 1.0, 1.0, 10.0)
    b.add_light(l)
    return (b.build() if build else b), meshes


def _nan(a, *at):
    a = np.array(a, F)
    a[at] = np.nan
    return a


def refusal_rows(frt, which):
    """[(row id, call, args)] for `which` in "scene", "renderer", "multi". The scene, the renderer or the multi renderer the rows run against holds
    pose_scene with a 2-joint skin and 2 morph targets bound to the quad and nothing bound to the strip. An argument is an int, None or a numpy array
    (its address is passed). The scene's rows begin with those against a scene that is not built."""
    from _skin_model import make_skin, make_palette
    from _morph_model import make_targets, make_weights
    pos = np.array(pose_meshes(frt)[QUAD].positions, F)
    att = np.array(pose_meshes(frt)[QUAD].attributes, F)
    pos5 = _nan(np.concatenate([pos, pos[:1]]), 2, 1)
    j, w = make_skin(4, 2)
    j5, w5 = np.concatenate([j, j[:1]]), _nan(np.concatenate([w, w[:1]]), 3, 0)
    pal, pal3 = make_palette(2), make_palette(3)
    tg, wt = make_targets(4, 2), make_weights(2)
    tg5 = _nan(make_targets(5, 2), 1, 4, 2)
    wt3 = make_weights(3)
    rows = [
        # ---- set_mesh_vertices
        ("vertices: bad id, null positions", "set_mesh_vertices", (BAD, None, None, 4)),
        ("vertices: wrong count, NaN position", "set_mesh_vertices", (QUAD, pos5, None, 5)),
        ("vertices: null positions, wrong count", "set_mesh_vertices", (QUAD, None, att, 5)),
        ("vertices: NaN position, NaN attributes", "set_mesh_vertices", (QUAD, _nan(pos, 3, 2), _nan(att, 1, 5), 4)),
        # ---- set_mesh_vertices_ex
        ("vertices_ex: device flag, unknown bit", "set_mesh_vertices_ex", (QUAD, pos, None, 4, DEV | UNK)),
        ("vertices_ex: unknown bit, bad id", "set_mesh_vertices_ex", (BAD, pos, None, 4, UNK | REC)),
        ("vertices_ex: device flag, bad id", "set_mesh_vertices_ex", (BAD, pos, None, 4, DEV)),
        ("vertices_ex: bad id, null positions", "set_mesh_vertices_ex", (BAD, None, None, 4, REC)),
        ("vertices_ex: wrong count, NaN position", "set_mesh_vertices_ex", (QUAD, pos5, None, 5, REC)),
        # ---- set_mesh_skin
        ("skin: bad id, null joints", "set_mesh_skin", (BAD, None, None, 0, 0)),
        ("skin: bad id, null weights", "set_mesh_skin", (BAD, j, None, 4, 2)),
        ("skin: null weights, wrong count", "set_mesh_skin", (QUAD, j, None, 5, 2)),
        ("skin: wrong count, NaN weight", "set_mesh_skin", (QUAD, j5, w5, 5, 2)),
        ("skin: no joints, a joint out of range", "set_mesh_skin", (QUAD, j, w, 4, 0)),
        ("skin: a joint out of range, a negative weight", "set_mesh_skin", (QUAD, j, -w, 4, 1)),
        # ---- set_mesh_pose
        ("pose: device flag, unknown bit", "set_mesh_pose", (QUAD, pal, 2, DEV | UNK)),
        ("pose: unknown bit, bad id", "set_mesh_pose", (BAD, pal, 2, UNK)),
        ("pose: device flag, bad id", "set_mesh_pose", (BAD, pal, 2, DEV | REC)),
        ("pose: bad id, null palette", "set_mesh_pose", (BAD, None, 2, 0)),
        ("pose: wrong count, NaN entry", "set_mesh_pose", (QUAD, _nan(pal3, 1, 7), 3, REC)),
        ("pose: wrong count, null palette", "set_mesh_pose", (QUAD, None, 3, 0)),
        ("pose: no skin, wrong count", "set_mesh_pose", (STRIP, pal3, 3, 0)),
        ("pose: no skin, null palette", "set_mesh_pose", (STRIP, None, 0, REC)),
        # ---- set_mesh_pose_ex
        ("pose_ex: device flag, unknown bit", "set_mesh_pose_ex", (QUAD, pal, 2, wt, 2, DEV | UNK)),
        ("pose_ex: unknown bit, bad id", "set_mesh_pose_ex", (BAD, pal, 2, wt, 2, UNK)),
        ("pose_ex: unknown bit, bad id, no weights", "set_mesh_pose_ex", (BAD, pal, 2, None, 0, UNK)),
        ("pose_ex: bad id, null palette, null weights", "set_mesh_pose_ex", (BAD, None, 2, None, 2, 0)),
        ("pose_ex: no skin, no targets", "set_mesh_pose_ex", (STRIP, pal, 2, wt, 2, 0)),
        ("pose_ex: no skin, wrong count, no weights", "set_mesh_pose_ex", (STRIP, pal3, 3, None, 0, REC)),
        ("pose_ex: NaN palette, NaN weight", "set_mesh_pose_ex", (QUAD, _nan(pal, 0, 3), 2, _nan(wt, 1), 2, 0)),
        ("pose_ex: wrong palette count, wrong weight count", "set_mesh_pose_ex", (QUAD, pal3, 3, wt3, 3, REC)),
        ("pose_ex: null palette, null weights", "set_mesh_pose_ex", (QUAD, None, 2, None, 2, 0)),
        ("pose_ex: wrong weight count, NaN weight", "set_mesh_pose_ex", (QUAD, pal, 2, _nan(wt3, 2), 3, 0)),
        ("pose_ex: null weights with a count", "set_mesh_pose_ex", (QUAD, pal, 2, None, 2, REC)),
        ("pose_ex: weights with no count", "set_mesh_pose_ex", (QUAD, pal, 2, _nan(wt, 0), 0, 0)),
        # ---- set_mesh_morph_targets
        ("targets: bad id, null deltas", "set_mesh_morph_targets", (BAD, None, 0, 0)),
        ("targets: bad id, no targets", "set_mesh_morph_targets", (BAD, tg, 4, 0)),
        ("targets: wrong count, NaN delta", "set_mesh_morph_targets", (QUAD, tg5, 5, 2)),
        ("targets: no targets, NaN delta", "set_mesh_morph_targets", (QUAD, _nan(tg, 0, 0, 0), 4, 0)),
        ("targets: too many targets, NaN delta", "set_mesh_morph_targets", (QUAD, _nan(tg, 0, 0, 0), 4, 4097)),
        # ---- set_mesh_morph_weights
        ("weights: device flag, unknown bit", "set_mesh_morph_weights", (QUAD, wt, 2, DEV | UNK)),
        ("weights: unknown bit, bad id", "set_mesh_morph_weights", (BAD, wt, 2, UNK | REC)),
        ("weights: device flag, bad id", "set_mesh_morph_weights", (BAD, wt, 2, DEV)),
        ("weights: bad id, null weights", "set_mesh_morph_weights", (BAD, None, 2, 0)),
        ("weights: wrong count, NaN weight", "set_mesh_morph_weights", (QUAD, _nan(wt3, 0), 3, REC)),
        ("weights: wrong count, null weights", "set_mesh_morph_weights", (QUAD, None, 3, 0)),
        ("weights: no targets, wrong count", "set_mesh_morph_weights", (STRIP, wt3, 3, 0)),
        ("weights: no targets, null weights", "set_mesh_morph_weights", (STRIP, None, 0, REC)),
    ]
    if which == "scene":      # the same calls against a scene that is not built: whatever else is wrong, that comes first
        unbuilt = [
            ("not built, vertices: bad id", "set_mesh_vertices", (BAD, pos, None, 4)),
            ("not built, vertices_ex: bad id, device flag", "set_mesh_vertices_ex", (BAD, pos, None, 4, DEV)),
            ("not built, skin: bad id", "set_mesh_skin", (BAD, j, w, 4, 2)),
            ("not built, pose: bad id, unknown bit", "set_mesh_pose", (BAD, pal, 2, UNK)),
            ("not built, pose_ex: bad id, NaN weight", "set_mesh_pose_ex", (BAD, pal, 2, _nan(wt, 0), 2, 0)),
            ("not built, targets: bad id", "set_mesh_morph_targets", (BAD, tg, 4, 2)),
            ("not built, weights: bad id, device flag", "set_mesh_morph_weights", (BAD, wt, 2, DEV)),
        ]
        rows = unbuilt + rows
    return rows


def bind_for_refusals(x):
    """The bindings refusal_rows assumes, on a scene, a renderer or a multi renderer over pose_scene."""
    from _skin_model import make_skin
    from _morph_model import make_targets
    x.set_mesh_skin(QUAD, *make_skin(4, 2), num_joints=2)
    x.set_mesh_morph_targets(QUAD, make_targets(4, 2))


def run_row(frt, prefix, handle, call, args):
    """(return code, message) of one row through the C call `prefix` + `call`."""
    lib = frt.lib()
    raw = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
    rc = getattr(lib, prefix + call)(handle, *raw)
    return rc, lib.frt_last_error().decode()
