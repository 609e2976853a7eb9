"""Moving instances from device memory, the parts that need no GPU (include/frt.h: frt_renderer_set_instance_transforms_ex, FRT_TRANSFORM_DEVICE; DESIGN.md
section 11, "Transforms from device memory"): the exports, the Python argument checks (on stand-ins that describe a device tensor, and on torch CPU tensors,
which are host arrays), and the arithmetic the kernels run (csrc/frt_instance_record.hpp), compiled here for the host and compared bit for bit with what
the library's own host functions leave in a scene."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("frt_renderer_set_instance_transforms_ex", "frt_renderer_transform_rejects")


def test_symbols_are_declared_and_exported(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    assert re.search(r"#define\s+FRT_TRANSFORM_DEVICE\s+1u", header)
    so = C.CDLL(os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib", "libfrt.so"))
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and getattr(frt.lib(), name).restype is C.c_int, name
    assert frt.TRANSFORM_DEVICE == 1
    assert not re.search(r"frt_multi_renderer_\w*(transforms_ex|transform_rejects)", header)      # (replicas on different devices: no multi form)


# ---- Python without a GPU ----
class _Dev:
    def __init__(self, index):
        self.index, self.type = index, "cuda"

    def __str__(self):
        return f"cuda:{self.index}"


class _Tensor:
    """What the argument checks look at of a device tensor, and nothing a device is needed for."""
    is_cuda = True

    def __init__(self, shape, dtype, contiguous=True, device=0):
        self.shape, self.dtype, self._c, self.device = tuple(shape), dtype, contiguous, _Dev(device)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        raise AssertionError("a refused call must not ask for the pointer")


_Tensor.__module__ = "torch"


class _NoLibrary:
    """A renderer whose handle must never be used: every check below has to refuse before the library is called."""
    device = 0
    _held = ()

    @property
    def _h(self):
        raise AssertionError("a refused call must not reach the library")


def test_argument_checks_need_no_device(frt):
    import torch
    from frt.renderer import Renderer, MultiRenderer, device_transform_args
    ids, mats = _Tensor((3,), torch.int32), _Tensor((3, 16), torch.float32)
    assert device_transform_args(torch, ids, mats, 0) == 3
    assert device_transform_args(torch, ids, _Tensor((3, 4, 4), torch.float32), 0) == 3
    assert device_transform_args(torch, _Tensor((0,), torch.int32), _Tensor((0, 16), torch.float32), 0) == 0
    host_ids, host_mats = np.arange(3), np.tile(np.eye(4, dtype=F).reshape(1, 16), (3, 1))
    bad = [(ids, host_mats), (host_ids, mats),                                                     # one of each kind
           (ids, _Tensor((3, 16), torch.float64)), (_Tensor((3,), torch.int64), mats),           # dtypes
           (_Tensor((3,), torch.int32, contiguous=False), mats), (ids, _Tensor((3, 16), torch.float32, contiguous=False)),
           (ids, _Tensor((3, 12), torch.float32)), (ids, _Tensor((48,), torch.float32)), (ids, _Tensor((3, 4, 4, 1), torch.float32)), (_Tensor((3, 1), torch.int32), mats),
           (ids, _Tensor((2, 16), torch.float32)),                                                 # counts differ
           (_Tensor((3,), torch.int32, device=1), mats), (ids, _Tensor((3, 16), torch.float32, device=1))]
    r = _NoLibrary()
    for i, m in bad:
        with pytest.raises(frt.FrtError):
            Renderer.set_instance_transforms(r, i, m)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        MultiRenderer.set_instance_transforms(r, ids, mats)
    with pytest.raises(frt.FrtError, match="host arrays only"):
        MultiRenderer.set_instance_transforms(r, host_ids, mats)


class _Handle:
    device, _h, _held = 0, 1234, []


class _Recorder:
    """Stands in for the library: records the calls made through it."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_host_arrays_and_cpu_tensors_take_the_host_call(frt, monkeypatch):
    import torch
    import frt.renderer as fr
    rec = _Recorder()
    monkeypatch.setattr(fr, "lib", lambda: rec)
    r = _Handle()
    m = np.tile(np.eye(4, dtype=F).reshape(1, 16), (2, 1))
    fr.Renderer.set_instance_transforms(r, [1, 2], m)
    fr.Renderer.set_instance_transforms(r, torch.tensor([1, 2], dtype=torch.int32), torch.from_numpy(m))      # CPU tensors are host arrays
    fr.Renderer.set_instance_transforms(r, torch.tensor([1, 2]), torch.from_numpy(m).reshape(2, 4, 4).double())
    assert [c[0] for c in rec.calls] == ["frt_renderer_set_instance_transforms"] * 3
    assert all(c[1][0] == 1234 and c[1][1] == 2 for c in rec.calls)


# ---- the shared arithmetic ----
@pytest.fixture(scope="module")
def record_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("instrec") / "libfrt_instrec.so")
    src = os.path.join(ROOT, "tests", "instrec", "frt_instance_record_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", src, "-o", out], check=True)
    L = C.CDLL(out)
    L.irc_batch.restype = None
    L.irc_batch.argtypes = [C.c_uint32] + [C.c_void_p] * 8
    return L


def _rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrices(n=10000, seed=20240611):
    """n column-major 4x4 (rows of 16 floats): rotation x scale x shear with scales from 1e-6 to 1e6, then the edge cases in fixed shares."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4, 4), np.float64)      # [k, column, row]
    for k in range(n):
        a = _rotation(rng) @ np.diag(10.0 ** rng.uniform(-6, 6, 3) if k % 2 else np.full(3, 10.0 ** rng.uniform(-6, 6))) @ _rotation(rng)
        kind = k % 10
        if kind == 3:                                   # mirrored: a negative determinant
            a = a @ np.diag([-1.0, 1.0, 1.0])
        elif kind == 5:                                 # near-singular: a column almost in the plane of the other two
            a[:, 2] = a[:, 0] * rng.uniform(-2, 2) + a[:, 1] * rng.uniform(-2, 2) + a[:, 2] * 10.0 ** rng.uniform(-12, -5)
        out[k, :3, :3] = a.T
        out[k, 3, :3] = rng.uniform(-50, 50, 3)
        out[k, 3, 3] = 1.0
    m = out.astype(F)
    for k in range(7, n, 10):                           # a determinant that is zero only in exact arithmetic: one column (or row) twice another, exactly, in f32
        if (k // 10) % 2:
            m[k, 1, :3] = m[k, 0, :3] * F(2.0)
        else:
            m[k, :3, 1] = m[k, :3, 0] * F(2.0)
    for k in range(9, n, 250):                          # exactly singular or not finite
        m[k, (k // 250) % 3, :3] = 0.0
    m[19, 0, 1] = np.nan; m[29, 3, 2] = np.inf; m[39, 2, 3] = -np.inf
    return m.reshape(n, 16)


def test_record_arithmetic_equals_the_host_functions(frt, record_check):
    """w2o, flip, the singular verdict and both light records of 10,000 matrices: the restatement the kernels run against frt_scene_set_instance_transforms
    (instance_inverse, quad_light_record, sphere_light_record), through a scene of one registered quad light and one registered sphere light. Equality."""
    g = frt.geometry
    b = frt.SceneBuilder()
    plane, sphere = b.add_mesh(g.create_plane()), b.add_mesh(g.create_sphere(0))
    eye = np.eye(4, dtype=F).reshape(16)
    em_q, em_s = np.array([1.0, 0.9, 0.8, 10.0], F), np.array([0.02, 0.3, 0.9, 7.5], F)
    b.register_quad_light(plane, eye, em_q[:3], float(em_q[3]))
    b.register_sphere_light(sphere, eye, em_s[:3], float(em_s[3]))
    b.build()
    m = matrices()
    n = m.shape[0]
    ok, w2o, flip = np.zeros(n, np.uint8), np.zeros((n, 9), F), np.zeros(n, np.uint32)
    quad, sph = np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint32)
    record_check.irc_batch(n, m.ctypes.data, em_q.ctypes.data, em_s.ctypes.data, ok.ctypes.data, w2o.ctypes.data, flip.ctypes.data, quad.ctypes.data, sph.ctypes.data)
    refused = mirrored = 0
    for k in range(n):
        try:
            b.set_instance_transforms([0, 1], [m[k], m[k]])
            accepted = True
        except frt.FrtError:
            accepted = False
        assert accepted == bool(ok[k]), f"matrix {k}: the scene {'accepts' if accepted else 'refuses'} it"
        if not accepted:
            refused += 1
            continue
        inst, lights = b.get("instances"), b.get("lights")
        assert inst[0, 5:21].tobytes() == m[k].tobytes()
        assert inst[0, 21:30].tobytes() == w2o[k].tobytes() and inst[1, 21:30].tobytes() == w2o[k].tobytes(), f"matrix {k}: w2o"
        assert inst[0, 4] == flip[k] == inst[1, 4], f"matrix {k}: flip"
        assert lights[0].tobytes() == quad[k].tobytes(), f"matrix {k}: quad light record"
        assert lights[1].tobytes() == sph[k].tobytes(), f"matrix {k}: sphere light record"
        mirrored += int(flip[k])
    assert refused >= 40 + 3 and mirrored >= 1000 and n - refused > 9000      # (the edge cases were met, on both sides of the verdict)
