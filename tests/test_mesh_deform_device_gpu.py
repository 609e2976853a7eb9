"""Deforming a mesh from device memory (include/frt.h: frt_renderer_set_mesh_vertices_ex, FRT_DEFORM_DEVICE; DESIGN.md section 11, "Vertices from device
memory"): torch tensors on the renderer's device give the replica and the frames that host arrays give; a tensor made on another stream just before the
call lands (the renderer's stream waits for the caller's); a non-finite float rejects the call on the device — nothing is applied, the reject counter
moves by one, the next call applies — and what cannot be a device call is refused on the host. Non-finite input is data here, not a crash case."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell_meshes
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_mesh_deform import deform, PLANE, SPHERE
from test_mesh_normals_gpu import REPLICA, W, H

pytestmark = pytest.mark.gpu
F = np.float32
EVERY = REPLICA + ("normals",)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda", 0)


def _replica(r):
    return {w: r.read_scene(w).tobytes() for w in EVERY}


def _up(torch, dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F)).to(dev)


@pytest.mark.parametrize("attrs,normals", [(False, "keep"), (True, "keep"), (False, "recompute"), (True, "recompute")],
                         ids=["positions", "attributes", "recompute", "attributes + recompute"])
def test_device_tensors_equal_host_arrays(gpu, torch_dev, attrs, normals):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    base = cornell_meshes(frt)
    a, b = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
    a.render(cam); b.render(cam)
    a.read_scene("normals"); b.read_scene("normals")      # (the pool of decoded normals exists: the calls keep it up)
    start = _replica(b)
    for m in (SPHERE, PLANE, SPHERE):                     # 642 vertices, 4, and the sphere again with no sync in between
        d = deform(frt, base[m], 0.6 + m)
        a.set_mesh_vertices(m, d.positions, d.attributes if attrs else None, normals=normals)
        b.set_mesh_vertices(m, _up(torch, dev, d.positions), _up(torch, dev, d.attributes) if attrs else None, normals=normals)
    got, want = _replica(b), _replica(a)
    for w in EVERY:
        assert got[w] == want[w], w
    assert got["tri_slots"] != start["tri_slots"] and b.deform_rejects() == 0
    a.clear(); b.clear()
    for f in range(2):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        compare_all(b.read_buffer, a.read_buffer, f, "device tensors vs host arrays")


def test_tensor_from_another_stream(gpu, torch_dev):
    """The positions are the result of kernels enqueued on a side stream just before the call, behind enough other work there that a call which did not
    wait for that stream would read the buffer before it is written (it holds zeros until then)."""
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    d = deform(frt, cornell_meshes(frt)[SPHERE], 1.1)
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H)
    a.set_mesh_vertices(SPHERE, d.positions, normals="recompute")
    src = _up(torch, dev, d.positions)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        busy = torch.ones((4096, 4096), device=dev)
        for _ in range(100):
            busy = busy * 1.0001 + 0.001
        pos = torch.zeros_like(src)
        pos += src * (busy[0, 0] * 0 + 1)                 # (depends on the work above; the same bits as `src`)
        b.set_mesh_vertices(SPHERE, pos, normals="recompute")
    got, want = _replica(b), _replica(a)
    for w in EVERY:
        assert got[w] == want[w], w


def test_non_finite_input_is_rejected_on_the_device(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    base = cornell_meshes(frt)
    r, ref = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE), frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights))
    assert r.deform_rejects() == 0
    d = deform(frt, base[SPHERE], 0.8)
    start = _replica(r)
    nan_pos = np.array(d.positions, F); nan_pos[641, 2] = np.nan              # the last vertex: the last, partial block of the validation launch
    inf_att = np.array(d.attributes, F); inf_att[300, 5] = np.inf
    for k, (p, a, normals) in enumerate([(nan_pos, None, "recompute"), (d.positions, inf_att, "keep"), (nan_pos, d.attributes, "keep")]):
        r.set_mesh_vertices(SPHERE, _up(torch, dev, p), _up(torch, dev, a), normals=normals)
        assert r.deform_rejects() == k + 1
        now = _replica(r)
        for w in EVERY:
            assert now[w] == start[w], f"rejected call {k}: {w} changed"
    # a bad call and a good one back to back, no sync: the good one applies fully, the counter moves by exactly one
    good = deform(frt, base[SPHERE], 1.3)
    r.set_mesh_vertices(SPHERE, _up(torch, dev, nan_pos), _up(torch, dev, inf_att), normals="recompute")
    r.set_mesh_vertices(SPHERE, _up(torch, dev, good.positions), _up(torch, dev, good.attributes), normals="recompute")
    ref.read_scene("normals")
    ref.set_mesh_vertices(SPHERE, good.positions, good.attributes, normals="recompute")
    assert r.deform_rejects() == 4
    got, want = _replica(r), _replica(ref)
    for w in EVERY:
        assert got[w] == want[w], w


def test_refusals(gpu, torch_dev):
    frt = gpu
    torch, dev = torch_dev
    fs = frt.scenes.create_cornell_box()
    d = deform(frt, cornell_meshes(frt)[SPHERE], 0.1)
    r = frt.Renderer(fs, W, H)
    start = _replica(r)
    pos, att = _up(torch, dev, d.positions), _up(torch, dev, d.attributes)
    bad = [(pos[:, :3].contiguous(), None), (pos.double(), None), (pos.t().contiguous().t(), None), (pos, att[:, :7].contiguous()), (pos, att.half()),
           (pos, d.attributes), (d.positions, att),                                  # one of each kind
           (pos[:-1].contiguous(), None), (pos, att[:-1].contiguous())]              # a wrong vertex count
    for p, a in bad:
        with pytest.raises(frt.FrtError):
            r.set_mesh_vertices(SPHERE, p, a)
    with pytest.raises(frt.FrtError, match="error -1"):
        r.set_mesh_vertices(99, pos)
    # (a tensor on another device needs a second device: on a one-GPU machine neither the Python check nor the library's `device != renderer's` check runs here)
    if torch.cuda.device_count() > 1:
        with pytest.raises(frt.FrtError, match="renderer on device 0"):
            r.set_mesh_vertices(SPHERE, pos.to(torch.device("cuda", 1)))
    multi = frt.MultiRenderer(fs, 64, 48, [0, 0])
    with pytest.raises(frt.FrtError, match="host arrays only"):
        multi.set_mesh_vertices(SPHERE, pos)
    n = pos.shape[0]
    assert frt.lib().frt_multi_renderer_set_mesh_vertices_ex(multi._h, SPHERE, pos.data_ptr(), None, n, frt.DEFORM_DEVICE) == -1
    assert frt.lib().frt_scene_set_mesh_vertices_ex(fs._h, SPHERE, pos.data_ptr(), None, n, frt.DEFORM_DEVICE) == -1
    host = np.ascontiguousarray(d.positions, F)
    assert frt.lib().frt_renderer_set_mesh_vertices_ex(r._h, SPHERE, host.ctypes.data, None, n, frt.DEFORM_DEVICE) == -1      # host memory is not device memory
    assert frt.lib().frt_renderer_set_mesh_vertices_ex(r._h, SPHERE, pos.data_ptr() + 4, None, n, frt.DEFORM_DEVICE) == -1     # not 16-byte aligned
    assert frt.lib().frt_renderer_set_mesh_vertices_ex(r._h, SPHERE, None, None, n, frt.DEFORM_DEVICE) == -1
    assert r.deform_rejects() == 0
    now = _replica(r)
    for w in EVERY:
        assert now[w] == start[w], w
