"""Cost of morphing a mesh (include/frt.h: frt_renderer_set_mesh_morph_weights, frt_renderer_set_mesh_pose_ex; DESIGN.md section 11, "Morph targets"): the
Cornell Box's sphere, the 82k-triangle blob and the colonnade's sphere mesh (tools/mesh_update_time.py: mesh_of), each under 4, 16 and 64 synthetic
targets. Five routes, every one with normals="recompute", microseconds per call (HIP events on the renderer's stream, median of 20; the call's host part
beside it):
  (a) numpy blend on the host, then set_mesh_vertices                       } what there was before the morph calls:
  (b) torch blend on the device, then set_mesh_vertices with device tensors } the baseline
  (c) set_mesh_morph_weights from host weights
  (d) set_mesh_morph_weights from a device tensor
  (e) set_mesh_pose with morph_weights: morph and skin (64 joints, tools/skin_time.py's synthetic skin), host inputs
and, for reference, the device-input positions-only set_mesh_vertices call with normals="recompute" that (c) and (d) are expected to cost plus one launch
plus the time to read 12 T n bytes. For (b) the events bracket the torch kernels as well (skin_time.py: call_us). Routes (a) to (d) must end in the same
triangle slots, and (e) in those of numpy morphing and skinning. One JSON line per scene and target count.
Usage: python tools/morph_time.py [cornell blob colonnade]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from mesh_update_time import mesh_of
from skin_time import synthetic_skin, palettes, numpy_skin, call_us

F = np.float32


def synthetic_targets(pos, ntargets, seed=0):
    """Smooth bumps: target t pushes the vertices near a random centre outwards by up to 5% of the mesh's size."""
    rng = np.random.default_rng(seed + ntargets)
    p = pos[:, :3].astype(np.float64)
    size = float(np.linalg.norm(p.max(0) - p.min(0)))
    d = np.empty((ntargets, len(p), 3), F)
    for t in range(ntargets):
        c = p[rng.integers(len(p))]
        fall = np.exp(-np.sum((p - c) ** 2, axis=1) / (0.15 * size) ** 2)
        d[t] = (0.05 * size * fall[:, None] * rng.standard_normal(3)[None, :]).astype(F)
    return d


def weight_sets(ntargets, count=2):
    return [np.random.default_rng(100 * ntargets + k).random(ntargets).astype(F) for k in range(count)]


def numpy_morph(pos, d, w):
    """The contract in float32 numpy (tests/_morph_model.py: morph_model)."""
    out = pos.copy()
    for t in range(len(w)):
        out[:, :3] = out[:, :3] + w[t] * d[t]
    return out


def torch_morph(pos, d, w):
    """The same chain of elementwise ops on the device (w: a device tensor; no read-back)."""
    out = pos.clone()
    for t in range(w.shape[0]):
        out[:, :3] = out[:, :3] + w[t] * d[t]
    return out


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
        j, sw = synthetic_skin(pos, 64)
        pals = palettes(64)
        for nt in (4, 16, 64):
            d = synthetic_targets(pos, nt)
            ws = weight_sets(nt)
            d_d, d_ws = torch.from_numpy(d).to(dev), [torch.from_numpy(w).to(dev) for w in ws]
            r.set_mesh_vertices(mesh, pos); r.set_mesh_morph_targets(mesh, d); r.set_mesh_skin(mesh, j, sw, num_joints=64); r.sync()
            k = [0]
            def route_a():
                k[0] ^= 1; r.set_mesh_vertices(mesh, numpy_morph(pos, d, ws[k[0]]), normals="recompute")
            def route_b():
                k[0] ^= 1; r.set_mesh_vertices(mesh, torch_morph(d_pos, d_d, d_ws[k[0]]), normals="recompute")
            def route_c():
                k[0] ^= 1; r.set_mesh_morph_weights(mesh, ws[k[0]])
            def route_d():
                k[0] ^= 1; r.set_mesh_morph_weights(mesh, d_ws[k[0]])
            def route_e():
                k[0] ^= 1; r.set_mesh_pose(mesh, pals[k[0]], morph_weights=ws[k[0]])
            routes = {}
            for key, fn, stream in (("a_numpy_then_set_mesh_vertices", route_a, rs), ("b_torch_then_set_mesh_vertices", route_b, cur),
                                    ("c_set_mesh_morph_weights_host", route_c, rs), ("d_set_mesh_morph_weights_device", route_d, rs),
                                    ("e_set_mesh_pose_morph_and_skin_host", route_e, rs)):
                fn(); r.sync()
                us, host = call_us(stream, rs, fn, r.sync)
                routes[key] = {"us": us, "us_host": host}
            # the routes end in the same replica
            route_c(); want = r.read_scene("tri_slots").tobytes()
            k[0] ^= 1; route_d(); same = r.read_scene("tri_slots").tobytes() == want
            k[0] ^= 1; route_a(); same = same and r.read_scene("tri_slots").tobytes() == want
            k[0] ^= 1; route_b(); same = same and r.read_scene("tri_slots").tobytes() == want
            k[0] ^= 1; route_e(); got = r.read_scene("tri_slots").tobytes()
            r.set_mesh_vertices(mesh, numpy_skin(numpy_morph(pos, d, ws[k[0]]), j, sw, pals[k[0]]), normals="recompute")
            same_e = r.read_scene("tri_slots").tobytes() == got
            print(json.dumps({"scene": name, "mesh_vertices": int(len(pos)), "targets": nt, "delta_bytes": int(d.nbytes),
                              "us_device_set_mesh_vertices_recompute": base[0], "us_host_device_set_mesh_vertices_recompute": base[1],
                              "routes": routes, "routes_agree": bool(same), "combined_agrees": bool(same_e), "deform_rejects": r.deform_rejects()}), flush=True)
        del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
