"""Moving instances of a built scene (include/frt.h: frt_scene_set_instance_transforms), on the host: the same tree with its
boxes refit, triangles / lights / instance records equal to a scene built from scratch with the new transforms, errors, no stale 8-wide tree,
and the oracle walking the refit tree agrees with its brute force."""
import ctypes as C
import numpy as np
import pytest

# Cornell Box instances (scenes.rs:50-130 order): 5 the quad light, 6 the glass crystal, 7 the sphere light, 8 the tall metal box
QUAD_LIGHT, CRYSTAL, SPHERE_LIGHT, TALL_BOX = 5, 6, 7, 8


def _frt_mats(frt):
    from frt.scenes import _T, _S, _RY, _RX, _mul
    return _T, _S, _RY, _RX, _mul


def cornell_moves(frt):
    """New transforms for the tall box, the sphere light, the quad light and (mirrored: negative determinant) the crystal."""
    _T, _S, _RY, _RX, _mul = _frt_mats(frt)
    S3 = lambda x, y, z: np.diag(np.array([x, y, z, 1.0], np.float32))
    return {TALL_BOX: _mul(_T(-0.2, -0.398, -0.1), _RY(0.9), S3(0.6, 1.2, 0.6)),
            SPHERE_LIGHT: _mul(_T(-0.3, 0.3, 0.2), _S(0.15)),
            QUAD_LIGHT: _mul(_T(0.2, 0.97, 0.1), _RX(np.pi), _S(0.4)),
            CRYSTAL: _mul(_T(0.3, -0.5, 0.35), S3(-0.5, 0.5, 0.5))}


def cornell_meshes(frt):
    g = frt.geometry
    return [g.create_plane(), g.create_cube(), g.create_sphere(3), g.create_crystal()]


def cornell(frt, moves=None):
    """The Cornell Box of scenes.rs issued call by call through the public builder, instance k with transform moves[k] where given."""
    moves = moves or {}
    ref = frt.scenes.create_cornell_box()
    inst, mats = ref.get("instances"), ref.get("materials")
    b = frt.SceneBuilder()
    for g in cornell_meshes(frt):
        b.add_mesh(g)
    for k in range(6):
        b.add_material(frt.Material.from_buffer_copy(np.ascontiguousarray(mats[k]).tobytes()))
    for k, row in enumerate(inst):
        m = np.asarray(moves[k], np.float32).reshape(16) if k in moves else row[5:21].view(np.float32)
        if k == QUAD_LIGHT:
            b.register_quad_light(int(row[0]), m, (1.0, 1.0, 1.0), 10.0)
        elif k == SPHERE_LIGHT:
            b.register_sphere_light(int(row[0]), m, (0.02, 0.02, 0.9), 10.0)
        else:
            b.add_instance(int(row[0]), int(row[1]), m)
    return b.build()


def move(scene, moves):
    ids = sorted(moves)
    scene.set_instance_transforms(ids, np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids]))
    return scene


def oracle_scene(orc, fs, meshes):
    """The oracle's own scene from the product scene's materials, lights and instances (nothing of its tree)."""
    from _oracle import OrcScene
    oh = orc.L.orc_scene_create()
    for g in meshes:
        pos = np.ascontiguousarray(g.positions, np.float32); att = np.ascontiguousarray(g.attributes, np.float32); idx = np.ascontiguousarray(g.indices, np.uint32)
        orc.L.orc_scene_add_mesh(oh, pos.ctypes.data, pos.shape[0], att.ctypes.data, idx.ctypes.data, idx.size)
    for row in fs.get("materials"):
        r = np.ascontiguousarray(row); orc.L.orc_scene_add_material(oh, r.ctypes.data)
    for row in fs.get("lights"):
        r = np.ascontiguousarray(row); orc.L.orc_scene_add_light(oh, r.ctypes.data)
    for row in fs.get("instances"):
        m = np.ascontiguousarray(row[5:21]); orc.L.orc_scene_add_instance(oh, int(row[0]), int(row[1]), m.ctypes.data)
    orc.L.orc_scene_build(oh)
    return OrcScene(orc, oh)


def by_id(slots):
    return slots[np.argsort(slots[:, 3].view(np.uint32), kind="stable")]


def _pad(tris):
    v0 = tris[:, 0:3]; v1 = v0 + tris[:, 3:6]; v2 = v0 + tris[:, 6:9]
    lo = np.minimum(np.minimum(v0, v1), v2); hi = np.maximum(np.maximum(v0, v1), v2)
    ext = np.float32(max(np.abs(lo).max(), np.abs(hi).max()))
    return lo, hi, np.float32(1e-4) * np.maximum(ext, np.float32(1.0))


def check_boxes(scene):
    """Every box of the binary, pair and quad trees equals the padded union of what lies below it (and so contains it)."""
    tris = scene.get("tris")
    lo, hi, pad = _pad(tris)
    slots = scene.get("tri_slots")
    sid = slots[:, 3].view(np.uint32)

    def leaf(ref):
        first, count = ref & 0xFFFFFF, (ref >> 24) & 0x7F
        ids = sid[first:first + count]
        return lo[ids].min(axis=0) - pad, hi[ids].max(axis=0) + pad

    nodes = scene.get("bvh2_nodes")
    bmin, bmax = nodes[:, 0:3].view(np.float32), nodes[:, 4:7].view(np.float32)
    left, count = nodes[:, 3], nodes[:, 7]
    order = scene.get("bvh2_tri_index")
    for i in range(len(nodes)):
        if count[i]:
            ids = order[left[i]:left[i] + count[i]]
            want = (lo[ids].min(axis=0) - pad, hi[ids].max(axis=0) + pad)
        else:
            c = [left[i], left[i] + 1]
            want = (np.minimum(bmin[c[0]], bmin[c[1]]), np.maximum(bmax[c[0]], bmax[c[1]]))
        assert np.array_equal(bmin[i], want[0]) and np.array_equal(bmax[i], want[1]), f"bvh2 node {i}"
    pairs = scene.get("pair_nodes")
    for i, p in enumerate(pairs):
        refs = p[12:14].view(np.uint32)
        for c in range(2):
            if refs[c] == 0xFFFFFFFF:
                continue
            if refs[c] & 0x80000000:
                want = leaf(refs[c])
            else:
                k = pairs[refs[c]]
                want = (np.minimum(k[[0, 4, 8]], k[[1, 5, 9]]), np.maximum(k[[2, 6, 10]], k[[3, 7, 11]]))
            got = (p[[c, 4 + c, 8 + c]], p[[2 + c, 6 + c, 10 + c]])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"pair node {i} child {c}"
    quads = scene.get("quad_nodes")
    for i, q in enumerate(quads):
        refs = q[24:28].view(np.uint32)
        for c in range(4):
            if refs[c] == 0xFFFFFFFF:
                continue
            if refs[c] & 0x80000000:
                want = leaf(refs[c])
            else:
                k = quads[refs[c]]; kr = k[24:28].view(np.uint32); v = kr != 0xFFFFFFFF
                want = (np.array([k[8 * a:8 * a + 4][v].min() for a in range(3)], np.float32), np.array([k[8 * a + 4:8 * a + 8][v].max() for a in range(3)], np.float32))
            got = (q[[c, 8 + c, 16 + c]], q[[4 + c, 12 + c, 20 + c]])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"quad node {i} child {c}"


SELECTORS = ("tris", "lights", "instances", "bvh2_nodes", "quad_nodes", "tri_slots", "pair_nodes", "instances_dev", "bvh2_tri_index")


def test_rebuilt_cornell_equals_the_factory(frt):
    """The test's call-by-call Cornell Box is the library's (so a fresh build with moved transforms is a fair reference)."""
    a, b = frt.scenes.create_cornell_box(), cornell(frt)
    for what in SELECTORS + ("materials",):
        assert a.get(what).tobytes() == b.get(what).tobytes(), what


@pytest.mark.parametrize("which", ["cornell", "restir"])
def test_same_transforms_change_nothing(frt, which):
    s = frt.scenes.create_cornell_box() if which == "cornell" else frt.scenes.create_restir_scene()
    before = {w: s.get(w).tobytes() for w in SELECTORS}
    inst = s.get("instances")
    s.set_instance_transforms(np.arange(len(inst)), inst[:, 5:21].view(np.float32).copy())
    for w in SELECTORS:
        assert s.get(w).tobytes() == before[w], w


def test_moved_cornell_matches_a_fresh_build(frt):
    moves = cornell_moves(frt)
    s = move(frt.scenes.create_cornell_box(), moves)
    fresh = cornell(frt, moves)
    for what in ("tris", "tri_instance", "lights", "instances", "instances_dev", "materials"):
        assert s.get(what).tobytes() == fresh.get(what).tobytes(), what
    assert by_id(s.get("tri_slots")).tobytes() == by_id(fresh.get("tri_slots")).tobytes()
    assert s.get("instances")[CRYSTAL, 4] == 1                          # mirrored: flip
    assert not np.array_equal(s.get("tris"), frt.scenes.create_cornell_box().get("tris"))
    # the tree is the original one, refit
    orig = frt.scenes.create_cornell_box()
    assert np.array_equal(s.get("bvh2_tri_index"), orig.get("bvh2_tri_index"))
    assert np.array_equal(s.get("bvh2_nodes")[:, [3, 7]], orig.get("bvh2_nodes")[:, [3, 7]])
    check_boxes(s)
    check_boxes(orig)


def test_lights_follow_their_instances(frt):
    s = frt.scenes.create_cornell_box()
    _T, _S, _RY, _RX, _mul = _frt_mats(frt)
    s.set_instance_transform(SPHERE_LIGHT, _mul(_T(-0.5, 0.25, 0.1), _S(0.2)))
    l = s.get("lights").view(np.float32)
    assert np.allclose(l[1, 0:3], (-0.5, 0.25, 0.1)) and np.isclose(l[1, 8], 0.1)     # sphere: position, radius = scale / 2
    q = s.get("lights")
    assert q[0].tobytes() == frt.scenes.create_cornell_box().get("lights")[0].tobytes()   # the quad light did not move


def test_add_light_lights_stay(frt, orc):
    import _scenes
    fs, _ = _scenes.bumpy_sphere_in_box(frt, orc, subdiv=2)
    before = fs.get("lights").tobytes()
    inst = fs.get("instances")
    m = inst[5, 5:21].view(np.float32).copy(); m[13] -= 0.1         # the light quad's instance, its light added with add_light
    fs.set_instance_transform(5, m)
    assert fs.get("lights").tobytes() == before
    check_boxes(fs)


def test_errors(frt):
    s = frt.scenes.create_cornell_box()
    before = {w: s.get(w).tobytes() for w in SELECTORS}
    eye = np.eye(4, dtype=np.float32)
    nan = eye.copy(); nan[3, 1] = np.nan
    sing = eye.copy(); sing[2, 2] = 0.0
    inf = eye.copy(); inf[0, 0] = np.inf
    for ids, mats in (([9], [eye]), ([0, 1000], [eye, eye]), ([0], [nan]), ([2], [sing]), ([0, 3], [eye, inf])):
        with pytest.raises(frt.FrtError):
            s.set_instance_transforms(ids, mats)
    with pytest.raises(frt.FrtError):
        s.set_instance_transforms([0, 1], [eye])                         # one matrix for two ids
    for w in SELECTORS:
        assert s.get(w).tobytes() == before[w], w                      # nothing applied
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.create_plane())
    b.add_instance(0, 0xFFFFFFFF, eye)
    with pytest.raises(frt.FrtError):
        b.set_instance_transforms([0], [eye])                           # not built
    assert b"not built" in frt.lib().frt_last_error()


def test_wide_tree_is_not_stale(frt):
    s = frt.scenes.create_cornell_box()
    s.get("wide8_nodes")                                                # made before the move
    old8 = s.get("tri_slots8")
    move(s, cornell_moves(frt))
    slots8 = s.get("tri_slots8")
    assert by_id(slots8).tobytes() == by_id(s.get("tri_slots")).tobytes()
    assert by_id(slots8).tobytes() != by_id(old8).tobytes()
    boxes = np.zeros(s.tree_stats()["wide8_nodes"] * 48, np.float32)
    assert frt.lib().frt_scene_get(s._h, 14, boxes.ctypes.data) == 0
    lo, hi, _ = _pad(s.get("tris"))
    b = boxes.reshape(-1, 8, 6)
    valid = b[:, :, 3] >= b[:, :, 0]
    assert b[valid][:, 0:3].min(axis=0).tolist() <= lo.min(axis=0).tolist()       # the root covers the moved triangles
    assert b[valid][:, 3:6].max(axis=0).tolist() >= hi.max(axis=0).tolist()


def test_oracle_over_the_refit_tree_matches_its_brute_force(frt, orc):
    from test_hostcheck_parity import compare_all
    moves = cornell_moves(frt)
    fs = move(frt.scenes.create_cornell_box(), moves)
    os_ = oracle_scene(orc, fs, cornell_meshes(frt))
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    W, H = 40, 30
    rb, rf = os_.renderer(W, H, 8, True, 8), os_.renderer(W, H, 8, False, 8)
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        rb.render(cam); rf.render(cam)
        compare_all(rb.read, rf.read, f, "refit tree vs brute force")
    sb, sf = rb.stats()["total"], rf.stats()["total"]
    assert (sb["closest"], sb["any"]) == (sf["closest"], sf["any"])
