"""Adding and removing instances of a built scene (include/frt.h: frt_scene_add_instances / _remove_instances), on the host: after
every call the scene equals, selector for selector, a scene built from scratch with the resulting instance list; the host ray queries report the new
ids; every refusal leaves every selector as it was; the new symbols are exported."""
import ctypes as C
import numpy as np
import pytest
from _instance_lists import assert_same_scene, snapshot, cornell_list, odd_list, two_instance_list, trs
from test_instance_update import QUAD_LIGHT, SPHERE_LIGHT, TALL_BOX, CRYSTAL

ERR_INVALID_ARG, ERR_STATE, ERR_LIMIT = -1, -4, -5
LISTS = {"cornell": cornell_list, "odd": odd_list, "two instances": two_instance_list}
TRI_MESH = {"cornell": 4, "odd": 1, "two instances": 0}      # the mesh the tests add instances of (one triangle; the plane where the scene has no other)


def removable(lst):
    return [k for k, e in enumerate(lst.entries) if e["kind"] == "inst"]


def new_instances(frt, which):
    return [TRI_MESH[which], 0], [0, len(LISTS[which](frt).materials) - 1], np.stack([trs(frt, (0.3, 0.2, 0.4), 0.3, 0.5), trs(frt, (-0.4, -0.3, 0.1), -0.25)])


@pytest.mark.parametrize("which", sorted(LISTS))
def test_remove_equals_a_scratch_build(frt, which):
    lst = LISTS[which](frt)
    ok = removable(lst)
    cases = {"first": [ok[0]], "last": [ok[-1]]}
    if len(ok) > 2:
        cases["middle"] = [ok[len(ok) // 2]]
        cases["several, one twice"] = [ok[-1], ok[0], ok[-1]]
    for name, ids in cases.items():
        s = lst.build(frt)
        s.get("wide8_nodes")                                  # (an 8-wide tree made before the call must not survive it)
        s.remove_instances(ids)
        assert_same_scene(frt, s, lst.removed(ids).build(frt), f"{which}, remove {name}")


@pytest.mark.parametrize("which", sorted(LISTS))
def test_add_equals_a_scratch_build(frt, which):
    lst = LISTS[which](frt)
    me, ma, m = new_instances(frt, which)
    s = lst.build(frt)
    n0 = s.counts()["instances"]
    assert s.add_instances(me, ma, m) == n0                   # the id of the first new instance
    after = lst.added(me, ma, m)
    assert_same_scene(frt, s, after.build(frt), f"{which}, add two")
    if which == "odd":
        assert lst.build(frt).counts()["tris"] == 15 and s.counts()["tris"] == 15 + 1 + 12      # odd; the one-triangle mesh, then mesh 0
    # add, then remove what was added: the scene it started from
    s.remove_instances([n0 + 1, n0])
    assert_same_scene(frt, s, lst.build(frt), f"{which}, add then remove")
    # ... and remove an old one after adding: the new instances shift down
    s.add_instances(me, ma, m)
    s.remove_instances([removable(lst)[0]])
    assert_same_scene(frt, s, after.removed([removable(lst)[0]]).build(frt), f"{which}, add then remove an older one")
    assert s.add_instances([], [], np.zeros((0, 16), np.float32)) == s.counts()["instances"]      # n == 0


def test_registered_light_keeps_its_link_and_moves_afterwards(frt):
    """Removing instances in front of a registered light renumbers its instance; the light must still follow that instance."""
    lst = cornell_list(frt)
    s = lst.build(frt)
    s.remove_instances([0, 3])
    m = trs(frt, (-0.3, 0.3, 0.2), 0.15)
    s.set_instance_transforms([SPHERE_LIGHT - 2], [m])
    want = lst.removed([0, 3]).moved(SPHERE_LIGHT - 2, m).build(frt)
    for w in ("tris", "tri_instance", "lights", "materials", "instances", "instances_dev", "shade_tris"):      # (a move keeps its tree: what does not depend on one)
        assert s.get(w).tobytes() == want.get(w).tobytes(), w
    assert s.get("lights").tobytes() != lst.removed([0, 3]).build(frt).get("lights").tobytes()
    with pytest.raises(frt.FrtError):
        s.set_instance_materials([QUAD_LIGHT - 2], [0])       # still known as a registered-light instance


def test_host_trace_reports_the_new_ids(frt):
    lst = cornell_list(frt)
    s = lst.build(frt)
    inst = s.get("instances")
    # a ray from the camera side straight at the tall box (instance 8): behind it the back wall (instance 2)
    o, d = np.array([[-0.35, -0.3, 2.5]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32)
    h = s.trace_closest(o, d)
    assert h["instance"][0] == TALL_BOX and inst[TALL_BOX][2] <= h["tri"][0] < inst[TALL_BOX][2] + inst[TALL_BOX][3]
    s.remove_instances([CRYSTAL])                              # in front of the box in the list: its ids shift down
    h2 = s.trace_closest(o, d)
    ntri = int(inst[CRYSTAL][3])
    assert h2["instance"][0] == TALL_BOX - 1 and h2["tri"][0] == h["tri"][0] - ntri and h2["primitive"][0] == h["primitive"][0]
    assert h2["t"].tobytes() == h["t"].tobytes()
    s.remove_instances([TALL_BOX - 1])                         # the box itself: the ray goes on to the back wall
    h3 = s.trace_closest(o, d)
    assert h3["instance"][0] == 2 and h3["t"][0] > h["t"][0] and h3["tri"][0] == inst[2][2] + h3["primitive"][0]
    want = lst.removed([CRYSTAL, TALL_BOX]).build(frt).trace_closest(o, d)
    for k in h3:
        assert h3[k].tobytes() == want[k].tobytes(), k


def _refused(frt, s, code, call):
    before = snapshot(frt, s)
    rc = call()
    assert rc == code, (rc, frt.lib().frt_last_error())
    assert snapshot(frt, s) == before, "a refused call changed the scene"


def test_refusals_change_nothing(frt):
    L = frt.lib()
    lst = cornell_list(frt)
    s = lst.build(frt)
    eye = np.eye(4, dtype=np.float32).reshape(1, 16)
    u32 = lambda *v: np.asarray(v, np.uint32)
    add = lambda me, ma, m, n=1: L.frt_scene_add_instances(s._h, n, me.ctypes.data if me is not None else None, ma.ctypes.data if ma is not None else None, m.ctypes.data if m is not None else None)
    rem = lambda ids, n=None: L.frt_scene_remove_instances(s._h, len(ids) if n is None else n, ids.ctypes.data if ids is not None else None)
    counts = s.counts()
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(None, u32(0), eye))
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), None, eye))
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), u32(0), None))
    _refused(frt, s, ERR_INVALID_ARG, lambda: rem(None, 1))
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(counts["meshes"]), u32(0), eye))
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), u32(counts["materials"]), eye))
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), u32(0xFFFFFFFF), eye))
    bad = eye.copy(); bad[0, 5] = np.nan
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), u32(0), bad))
    flat = eye.copy(); flat[0, 10] = 0.0
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0), u32(0), flat))
    two = np.concatenate([eye, flat])                          # the first of two is fine: nothing of it may be applied
    _refused(frt, s, ERR_INVALID_ARG, lambda: add(u32(0, 0), u32(0, 0), two, 2))
    _refused(frt, s, ERR_INVALID_ARG, lambda: rem(u32(counts["instances"])))
    _refused(frt, s, ERR_INVALID_ARG, lambda: rem(u32(0, counts["instances"])))
    _refused(frt, s, ERR_INVALID_ARG, lambda: rem(u32(QUAD_LIGHT)))
    _refused(frt, s, ERR_INVALID_ARG, lambda: rem(u32(0, SPHERE_LIGHT)))
    assert b"light" in L.frt_last_error()
    # n == 0
    assert add(None, None, None, 0) == counts["instances"] and rem(None, 0) == 0
    # removing every instance (of a scene without registered lights, so that nothing else refuses first), with a duplicate
    t = two_instance_list(frt).build(frt)
    before = snapshot(frt, t)
    every = u32(1, 0, 1)
    assert L.frt_scene_remove_instances(t._h, 3, every.ctypes.data) == ERR_INVALID_ARG
    assert snapshot(frt, t) == before
    # not built
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.create_plane()); b.add_material(frt.material_new([1, 1, 1, 1])); b.add_instance(0, 0, eye)
    zero = u32(0)
    assert L.frt_scene_add_instances(b._h, 1, zero.ctypes.data, zero.ctypes.data, eye.ctypes.data) == ERR_STATE
    assert L.frt_scene_remove_instances(b._h, 1, zero.ctypes.data) == ERR_STATE
    assert L.frt_scene_add_instances(None, 0, None, None, None) == ERR_INVALID_ARG


def test_triangle_limit(frt):
    """0xFFFFFFFE triangles is the limit; it is checked on the sum, in 64 bits, before anything is built. A mesh of 2^20 triangles whose instance is
    asked for 4096 times would make 2^32 (a 32-bit sum would wrap to the scene's own count and pass)."""
    n = 1 << 20
    pos = np.zeros((3, 4), np.float32); pos[:, 3] = 1.0; pos[1, 0] = pos[2, 1] = 1.0
    att = np.zeros((3, 8), np.float32)
    b = frt.SceneBuilder()
    b.add_mesh(frt.geometry.Geometry(pos, att, np.arange(3, dtype=np.uint32)))
    b.add_mesh(frt.geometry.Geometry(pos, att, np.tile(np.arange(3, dtype=np.uint32), n)))
    b.add_material(frt.material_new([1, 1, 1, 1]))
    b.add_instance(0, 0, np.eye(4, dtype=np.float32))
    b.build()
    before = snapshot(frt, b)
    k = 4096
    me, ma, m = np.ones(k, np.uint32), np.zeros(k, np.uint32), np.tile(np.eye(4, dtype=np.float32).reshape(16), (k, 1))
    rc = frt.lib().frt_scene_add_instances(b._h, k, me.ctypes.data, ma.ctypes.data, m.ctypes.data)
    assert rc == ERR_LIMIT, frt.lib().frt_last_error()
    assert snapshot(frt, b) == before


def test_python_packers(frt):
    s = two_instance_list(frt).build(frt)
    with pytest.raises(frt.FrtError):
        s.add_instances([0, 0], [0], np.zeros((2, 16), np.float32))
    with pytest.raises(frt.FrtError):
        s.add_instances([0], [0], np.zeros((2, 16), np.float32))
    with pytest.raises(frt.FrtError):
        s.remove_instances([-1])
    assert s.add_instances(0, 0, trs(frt, (0.0, 0.4, 0.0), 0.3)) == 2      # ints and one matrix
    s.remove_instances(2)
    assert s.counts()["instances"] == 2


def test_new_symbols_are_exported_and_declared(frt):
    import os
    names = ["frt_scene_add_instances", "frt_scene_remove_instances", "frt_renderer_add_instances", "frt_renderer_remove_instances", "frt_renderer_scene_counts",
             "frt_multi_renderer_add_instances", "frt_multi_renderer_remove_instances"]
    L = C.CDLL(os.path.abspath(frt._lib.LIB_PATH))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frt.h")).read()
    for n in names:
        assert hasattr(L, n), f"{n} is not exported"
        assert n + "(" in header and n in frt._lib.SYMBOLS
