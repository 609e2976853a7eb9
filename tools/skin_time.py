"""Cost of posing a skinned mesh (include/frt.h: frt_renderer_set_mesh_pose; DESIGN.md section 11, "Skinning"): the Cornell Box's sphere, the
82k-triangle blob and the colonnade's sphere mesh (tools/mesh_update_time.py: mesh_of), each under synthetic skins of 4, 64 and 256 joints. Four routes
to the same replica, every one with normals="recompute", microseconds per call (HIP events on the renderer's stream, median of 20; the call's host part
beside it):
  (a) numpy skinning on the host, then set_mesh_vertices                       } what there was before set_mesh_pose:
  (b) torch skinning on the device, then set_mesh_vertices with device tensors } the baseline
  (c) set_mesh_pose from host matrices
  (d) set_mesh_pose from a device tensor
and, for reference, the device-input positions-only set_mesh_vertices call with normals="recompute" that (d) is expected to cost plus one launch.
For (b) the events bracket the torch kernels as well: they run on the caller's stream, which the renderer's stream waits for, so the first event is
recorded on the caller's stream there and the last on the renderer's. One JSON line per scene and joint count. Usage: python tools/skin_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from mesh_update_time import mesh_of

F = np.float32


def synthetic_skin(pos, njoints, seed=0):
    """Joints by position along y (neighbouring vertices share joints, as a rig's do) plus three random neighbours; weights normalised in float32."""
    rng = np.random.default_rng(seed + njoints)
    n = len(pos)
    y = pos[:, 1].astype(np.float64)
    t = (y - y.min()) / max(y.max() - y.min(), 1e-9)
    main = np.minimum((t * njoints).astype(np.int64), njoints - 1)
    j = np.stack([main] + [np.clip(main + rng.integers(-2, 3, n), 0, njoints - 1) for _ in range(3)], axis=1).astype(np.uint16)
    w = rng.random((n, 4)).astype(F) + F(0.05)
    return j, (w / w.sum(axis=1, keepdims=True)).astype(F)


def palettes(njoints, count=2):
    out = []
    for k in range(count):
        rng = np.random.default_rng(100 * njoints + k)
        m = np.tile(np.eye(4, dtype=F).reshape(1, 16), (njoints, 1))
        m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] += (0.03 * rng.standard_normal((njoints, 9))).astype(F)
        m[:, 12:15] = (0.01 * rng.standard_normal((njoints, 3))).astype(F)
        out.append(m)
    return out


def numpy_skin(pos, j, w, m):
    """The contract in float32 numpy (tests/_skin_model.py: skin_model)."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    out = pos.copy()
    for r in range(3):
        q = [((m[j[:, k], r] * x + m[j[:, k], 4 + r] * y) + m[j[:, k], 8 + r] * z) + m[j[:, k], 12 + r] for k in range(4)]
        out[:, r] = ((w[:, 0] * q[0] + w[:, 1] * q[1]) + w[:, 2] * q[2]) + w[:, 3] * q[3]
    return out


def torch_skin(pos, j, w, m):
    """The same chain of elementwise ops on the device (j: int64 [n, 4])."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    out = pos.clone()
    for r in range(3):
        q = [((m[j[:, k], r] * x + m[j[:, k], 4 + r] * y) + m[j[:, k], 8 + r] * z) + m[j[:, k], 12 + r] for k in range(4)]
        out[:, r] = ((w[:, 0] * q[0] + w[:, 1] * q[1]) + w[:, 2] * q[2]) + w[:, 3] * q[3]
    return out


def call_us(first, last, call, sync, reps=20):
    """(median HIP-event microseconds from an event on stream `first` in front of the call to one on stream `last` behind it, median host microseconds)"""
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(first)
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e6)
        b.record(last)
        sync()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(dev)), 1), round(float(np.median(host)), 1)


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 256, 144      # (no frame is timed here: the frame after a deformation is tools/mesh_update_time.py's)
    for name in names:
        fs, _ = scene_of(name, orc)
        mesh, geo = mesh_of(name)
        pos = np.ascontiguousarray(geo.positions, F)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        dev = torch.device("cuda", r.device)
        rs = torch.cuda.ExternalStream(r.stream_handle(0))
        cur = torch.cuda.current_stream(dev)
        d_pos = torch.from_numpy(pos).to(dev)
        r.set_mesh_vertices(mesh, pos, normals="recompute"); r.sync()      # (the one-time adjacency build is not part of a call's steady cost)
        base = call_us(rs, rs, lambda: r.set_mesh_vertices(mesh, d_pos, normals="recompute"), r.sync)
        for nj in (4, 64, 256):
            j, w = synthetic_skin(pos, nj)
            pals = palettes(nj)
            d_j, d_w, d_pals = torch.from_numpy(j.astype(np.int64)).to(dev), torch.from_numpy(w).to(dev), [torch.from_numpy(m).to(dev) for m in pals]
            r.set_mesh_vertices(mesh, pos); r.set_mesh_skin(mesh, j, w, num_joints=nj); r.sync()
            k = [0]
            def route_a():
                k[0] ^= 1; r.set_mesh_vertices(mesh, numpy_skin(pos, j, w, pals[k[0]]), normals="recompute")
            def route_b():
                k[0] ^= 1; r.set_mesh_vertices(mesh, torch_skin(d_pos, d_j, d_w, d_pals[k[0]]), normals="recompute")
            def route_c():
                k[0] ^= 1; r.set_mesh_pose(mesh, pals[k[0]])
            def route_d():
                k[0] ^= 1; r.set_mesh_pose(mesh, d_pals[k[0]])
            routes = {}
            for key, fn, stream in (("a_numpy_then_set_mesh_vertices", route_a, rs), ("b_torch_then_set_mesh_vertices", route_b, cur),
                                    ("c_set_mesh_pose_host", route_c, rs), ("d_set_mesh_pose_device", route_d, rs)):
                fn(); r.sync()
                us, host = call_us(stream, rs, fn, r.sync)
                routes[key] = {"us": us, "us_host": host}
            # the four routes end in the same replica
            route_c(); want = r.read_scene("tri_slots").tobytes()
            k[0] ^= 1; route_d(); same = r.read_scene("tri_slots").tobytes() == want
            k[0] ^= 1; route_a(); same = same and r.read_scene("tri_slots").tobytes() == want
            print(json.dumps({"scene": name, "mesh_vertices": int(len(pos)), "joints": nj, "palette_bytes": nj * 64,
                              "us_device_set_mesh_vertices_recompute": base[0], "us_host_device_set_mesh_vertices_recompute": base[1],
                              "routes": routes, "routes_agree": bool(same), "deform_rejects": r.deform_rejects()}), flush=True)
        del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
