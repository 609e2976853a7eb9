"""Moving instances from device memory (include/frt.h: frt_renderer_set_instance_transforms_ex, FRT_TRANSFORM_DEVICE; DESIGN.md section 11, "Transforms
from device memory"): ids and matrices given as torch tensors on the renderer's device leave the replica, byte for byte, and the frames as the same ids and
matrices given as host arrays do — instance records, linked lights, triangle slots and both trees; a tensor made on another stream just before the call
lands; a bad id, a non-finite entry or a singular 3x3 rejects the whole call on the device (nothing applied, the counter moves by one, the next call
applies); the calls that read the host's mirror of the matrices afterwards see the moved ones; and what cannot be a device call is refused on the host.
Bad input is data here, not a crash case."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_moves, cornell_meshes, QUAD_LIGHT, CRYSTAL, SPHERE_LIGHT, TALL_BOX
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform
from test_mesh_normals_gpu import REPLICA, W, H

pytestmark = pytest.mark.gpu
F = np.float32
EVERY = REPLICA + ("instances_dev", "lights", "materials")


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda", 0)


def _replica(r, skip=()):
    return {w: r.read_scene(w).tobytes() for w in EVERY if w not in skip}


def _same(b, a, what, skip=()):
    got, want = _replica(b, skip), _replica(a, skip)
    for w in want:
        assert got[w] == want[w], f"{what}: {w}"
    return got


def _flat(mats):
    return np.ascontiguousarray(np.stack([np.asarray(m, F).reshape(16) for m in mats]))


def _move(torch, dev, host, device, ids, mats, square=False):
    """The same call on both: host arrays to `host`, tensors to `device` ([n, 4, 4] instead of [n, 16] when `square`)."""
    m = _flat(mats)
    host.set_instance_transforms(list(ids), m)
    t = torch.from_numpy(m.reshape(-1, 4, 4) if square else m).to(dev)
    device.set_instance_transforms(torch.tensor(list(ids), dtype=torch.int32, device=dev), t)


def _shifted(fs, k, delta):
    m = fs.get("instances")[k, 5:21].view(F).copy()
    m[12:15] += np.asarray(delta, F)
    return m


def _calls(frt, fs, case):
    mv = cornell_moves(frt)
    n = len(fs.get("instances"))
    if case == "one instance":
        return [([TALL_BOX], [mv[TALL_BOX]])]
    if case == "all instances":
        return [(list(range(n)), [mv[k] if k in mv else _shifted(fs, k, (0.01 * k, -0.02, 0.005 * k)) for k in range(n)])]
    if case == "an id given twice":
        return [([TALL_BOX, CRYSTAL, TALL_BOX], [_shifted(fs, TALL_BOX, (0.3, 0.0, 0.0)), mv[CRYSTAL], mv[TALL_BOX]])]
    if case == "600 records of 9 instances":      # three blocks of records: the last writer of an instance is found across blocks
        ids = [(7 * k) % n for k in range(600)]
        return [(ids, [_shifted(fs, i, (0.0003 * k, 0.0, -0.0002 * k)) for k, i in enumerate(ids)])]
    if case == "mirrored":
        return [([CRYSTAL], [mv[CRYSTAL]])]
    assert case == "two calls, no sync"
    return [([TALL_BOX, QUAD_LIGHT], [_shifted(fs, TALL_BOX, (0.2, 0.0, 0.1)), mv[QUAD_LIGHT]]), ([SPHERE_LIGHT, TALL_BOX], [mv[SPHERE_LIGHT], mv[TALL_BOX]])]


@pytest.mark.parametrize("case", ["one instance", "all instances", "an id given twice", "600 records of 9 instances", "mirrored", "two calls, no sync"])
def test_device_tensors_equal_host_arrays(gpu, torch_dev, case):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    a.render(cam); b.render(cam)
    start = _replica(b)
    for k, (ids, mats) in enumerate(_calls(frt, fs, case)):
        _move(torch, dev, a, b, ids, mats, square=bool(k % 2))
    got = _same(b, a, case)
    assert got["tri_slots"] != start["tri_slots"] and b.transform_rejects() == 0
    if case == "mirrored":
        flip = lambda raw: np.frombuffer(raw, np.uint32).reshape(-1, 16)[CRYSTAL, 3]
        assert flip(got["instances_dev"]) != flip(start["instances_dev"])
    a.clear(); b.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "device tensors vs host arrays")
    _same(b, a, case + ", after the frames")


def _sphere_light_scene(frt):
    from frt.scenes import _T, _S, _RX, _mul
    g = frt.geometry
    b = frt.SceneBuilder()
    plane, ball = b.add_mesh(g.create_plane()), b.add_mesh(g.create_sphere(1))
    grey = b.add_material(frt.material_new([0.7, 0.7, 0.7, 1.0]))
    b.add_instance(plane, grey, _mul(_T(0.0, -1.0, 0.0), _S(4.0)))
    b.register_quad_light(plane, _mul(_T(0.0, 1.5, 0.0), _RX(np.pi), _S(0.5)), (1.0, 1.0, 1.0), 10.0)
    b.add_instance(ball, grey, _mul(_T(-0.6, -0.5, 0.0), _S(0.5)))
    b.register_sphere_light(ball, _mul(_T(0.5, 0.2, 0.1), _S(0.2)), (0.9, 0.4, 0.1), 6.0)
    return b.build()


def test_linked_lights_move_with_their_instances(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    from frt.scenes import _T, _S, _RY, _mul
    mv = cornell_moves(frt)
    small = _sphere_light_scene(frt)
    for fs, ids, mats in ((frt.scenes.create_cornell_box(), [QUAD_LIGHT], [mv[QUAD_LIGHT]]),
                          (frt.scenes.create_cornell_box(), [SPHERE_LIGHT, QUAD_LIGHT], [mv[SPHERE_LIGHT], mv[QUAD_LIGHT]]),
                          (small, [3, 1], [_mul(_T(-0.2, 0.4, 0.3), _RY(0.4), _S(0.35)), _mul(_T(0.1, 1.4, 0.0), _RY(0.3), np.diag(np.array([0.4, -0.4, 0.7, 1.0], F)))])):
        a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
        start = _replica(b)
        _move(torch, dev, a, b, ids, [_shifted(fs, k, (0.05, 0.0, -0.05)) for k in ids])
        for x in (a, b, fs):                                   # (the record of a light moved afterwards carries the emission as it is now)
            x.set_light_emission(0, (0.5, 0.25, 1.0), 3.0)
        _move(torch, dev, a, b, ids, mats)
        got = _same(b, a, "linked lights")
        assert got["lights"] != start["lights"] and got["instances_dev"] != start["instances_dev"] and b.transform_rejects() == 0
        fs.set_instance_transforms(ids, _flat(mats))           # the host specification itself
        assert got["lights"] == fs.get("lights").tobytes() and got["instances_dev"] == fs.get("instances_dev").tobytes()


def test_tensors_from_another_stream(gpu, torch_dev):
    """The matrices are the result of kernels enqueued on a side stream just before the call, behind enough other work there that a call which did not
    wait for that stream would read the buffer before it is written (it holds zeros until then: singular matrices, a rejected call)."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    mv = cornell_moves(frt)
    ids = sorted(mv)
    m = _flat([mv[k] for k in ids])
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    a.set_instance_transforms(ids, m)
    src = torch.from_numpy(m).to(dev)
    idt = torch.tensor(ids, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        busy = torch.ones((4096, 4096), device=dev)
        for _ in range(100):
            busy = busy * 1.0001 + 0.001
        mats = torch.zeros_like(src)
        mats += src * (busy[0, 0] * 0 + 1)                # (depends on the work above; the same bits as `src`)
        b.set_instance_transforms(idt, mats)
    _same(b, a, "another stream")
    assert b.transform_rejects() == 0


def test_bad_input_is_rejected_on_the_device(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    mv = cornell_moves(frt)
    n = len(fs.get("instances"))
    r, ref = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    assert r.transform_rejects() == 0
    start = _replica(r)
    ids = [TALL_BOX, CRYSTAL, QUAD_LIGHT]
    good = _flat([mv[k] for k in ids])
    nan = good.copy(); nan[2, 13] = np.nan                 # in the translation of the last record
    inf = good.copy(); inf[0, 5] = np.inf
    sing = good.copy(); sing[1, 4:8] = 0.0                 # a zero column
    up = lambda i, m: (torch.tensor(i, dtype=torch.int32, device=dev), torch.from_numpy(m).to(dev))
    for k, (i, m) in enumerate([(ids, nan), (ids, inf), (ids, sing), ([TALL_BOX, n, QUAD_LIGHT], good)]):
        r.set_instance_transforms(*up(i, m))
        assert r.transform_rejects() == k + 1
        now = _replica(r)
        for w in EVERY:
            assert now[w] == start[w], f"rejected call {k}: {w} changed"
    # far out of range, and a bad call and a good one back to back with no sync: the good one applies fully, the counter moves by one per bad call
    r.set_instance_transforms(*up([0xFFFFFFFF - (1 << 32), TALL_BOX, 1 << 30], good))
    r.set_instance_transforms(*up(ids, good))
    ref.set_instance_transforms(ids, good)
    assert r.transform_rejects() == 5
    _same(r, ref, "the good call after the rejected ones")


def test_calls_that_read_the_matrix_mirror(gpu, torch_dev):
    """After a device move the host's copy of the matrices is stale: the calls that read it (a deformation of the moved instance's mesh, add_instances and
    remove_instances, which carry every instance's record over) must see the moved matrix, as they do after the same move from host arrays."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    mv = cornell_moves(frt)
    inst = fs.get("instances")
    mesh, mat = int(inst[TALL_BOX, 0]), int(inst[TALL_BOX, 1])
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    a.render(cam); b.render(cam)
    _move(torch, dev, a, b, [TALL_BOX, CRYSTAL], [mv[TALL_BOX], mv[CRYSTAL]])
    _same(b, a, "the move")
    d = deform(frt, cornell_meshes(frt)[mesh], 0.4)
    for x in (a, b):
        x.set_mesh_vertices(mesh, d.positions, d.attributes)
    _same(b, a, "set_mesh_vertices after the move")
    _move(torch, dev, a, b, [TALL_BOX], [_shifted(fs, TALL_BOX, (0.1, 0.0, 0.2))])      # (the mirror is stale again when add_instances reads it)
    new = _shifted(fs, CRYSTAL, (-0.5, 0.3, -0.2))
    assert a.add_instances([mesh], [mat], [new]) == b.add_instances([mesh], [mat], [new]) == len(inst)
    _same(b, a, "add_instances after the move", skip=("pair_nodes",))               # (the pair tree is not rebuilt)
    _move(torch, dev, a, b, [len(inst), TALL_BOX], [_shifted(fs, CRYSTAL, (-0.4, 0.2, -0.2)), mv[TALL_BOX]])
    for x in (a, b):
        x.remove_instances([2])
    moved = TALL_BOX - 1
    _same(b, a, "remove_instances after the move", skip=("pair_nodes",))
    for x in (a, b):
        x.rebuild_tree("sah")
    _same(b, a, "rebuild_tree", skip=("pair_nodes",))
    _move(torch, dev, a, b, [moved, QUAD_LIGHT - 1], [_shifted(fs, TALL_BOX, (-0.1, 0.05, 0.1)), mv[QUAD_LIGHT]])
    _same(b, a, "the second move", skip=("pair_nodes",))
    assert b.transform_rejects() == 0
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)
    ha, hb = a.pick(cam, xy), b.pick(cam, xy)
    on = ha["instance"][ha["tri"] != 0xFFFFFFFF] == moved
    assert on.any() and np.array_equal(ha["instance"], hb["instance"]) and np.array_equal(ha["tri"], hb["tri"])
    # and the other way round: a host-array move after device moves is the truth the next device move builds on
    for x in (a, b):
        x.set_instance_transforms([moved], _flat([_shifted(fs, TALL_BOX, (0.0, 0.1, 0.0))]))
    _move(torch, dev, a, b, [CRYSTAL - 1], [_shifted(fs, CRYSTAL, (0.1, 0.1, 0.1))])
    for x in (a, b):
        x.set_mesh_vertices(mesh, d.positions)
    _same(b, a, "host move, device move, deformation", skip=("pair_nodes",))


def test_refusals_on_the_host(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    mv = cornell_moves(frt)
    r = frt.Renderer(fs, W, H)
    start = _replica(r)
    m = _flat([mv[TALL_BOX], mv[CRYSTAL]])
    ids, mats = torch.tensor([TALL_BOX, CRYSTAL], dtype=torch.int32, device=dev), torch.from_numpy(m).to(dev)
    wide = torch.zeros((2, 32), dtype=torch.float32, device=dev)
    bad = [(ids, m), ([TALL_BOX, CRYSTAL], mats),                                        # one of each kind
           (ids, mats.double()), (ids.long(), mats),                                     # float64 matrices, int64 ids
           (ids, wide[:, :16]), (torch.zeros((2, 2), dtype=torch.int32, device=dev)[:, 0], mats),      # not contiguous
           (ids, mats[:, :12].contiguous()), (ids, mats.reshape(32)), (ids[:1], mats), (ids.reshape(2, 1), mats)]      # wrong shapes
    for i, t in bad:
        with pytest.raises(frt.FrtError):
            r.set_instance_transforms(i, t)
    multi = frt.MultiRenderer(fs, 64, 48, [0, 0])
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_instance_transforms(ids, mats)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    with pytest.raises(frt.FrtError):
        r.set_instance_transforms(ids, mats)                  # a frame is open
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    L, D = frt.lib(), frt.TRANSFORM_DEVICE
    assert L.frt_renderer_set_instance_transforms_ex(r._h, 2, ids.data_ptr(), mats.data_ptr(), 2) == -1                    # an unknown flag bit
    assert L.frt_renderer_set_instance_transforms_ex(r._h, 2, ids.data_ptr(), m.ctypes.data, D) == -1                      # host memory is not device memory
    assert L.frt_renderer_set_instance_transforms_ex(r._h, 2, ids.data_ptr(), mats.data_ptr() + 4, D) == -1                # not 16-byte aligned
    assert L.frt_renderer_set_instance_transforms_ex(r._h, 2, None, mats.data_ptr(), D) == -1
    assert r.transform_rejects() == 0
    now = _replica(r)
    for w in EVERY:
        assert now[w] == start[w], w
    host = np.array([TALL_BOX, CRYSTAL], np.uint32)
    assert L.frt_renderer_set_instance_transforms_ex(r._h, 2, host.ctypes.data, m.ctypes.data, 0) == 0                     # without the flag: the host call
    ref = frt.Renderer(fs, W, H)
    ref.set_instance_transforms([TALL_BOX, CRYSTAL], m)
    _same(r, ref, "flags == 0")
