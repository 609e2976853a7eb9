"""Cost of deforming a mesh (include/frt.h: frt_renderer_set_mesh_vertices; DESIGN.md section 11, "Deforming meshes"): the Cornell Box's sphere
(1,280 triangles, one instance), the 82k-triangle blob and the colonnade's sphere mesh (5,120 triangles, 48 instances) (tests/_scenes.py):
microseconds per call with and without attributes (HIP events on the renderer's stream, median of 20; the call's host part, which copies the
vertices into pinned memory, is reported beside it), the set_instance_transforms call for the same instances, the frame time before and after
(1920x1080, two-stream schedule), and the host rebuild + renderer re-create the call replaces.
Then the routes to correct normals and to device-resident vertices ("Recomputed normals", "Vertices from device memory"), each
timed the same way with the frame time after it: (a) smooth normals computed on the host in numpy, encoded, and passed as attributes — the only route
before normals="recompute"; (b) host positions with normals="recompute"; (c) device tensors, normals="keep"; (d) device tensors, normals="recompute".
One JSON line per scene. Usage: python tools/mesh_update_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of, frame_ms


def mesh_of(name):
    """(mesh id, its geometry as the scene was built with it)"""
    g = frt.geometry
    if name == "cornell":
        return 2, g.create_sphere(3)
    if name == "colonnade":
        return 2, g.create_sphere(4)
    s = g.create_sphere(6)                                  # tests/_scenes.py: bumpy_sphere_in_box
    p = s.positions[:, :3].astype(np.float64) * 2.0
    disp = 1.0 + 0.08 * np.sin(7.0 * p[:, 0]) * np.sin(5.0 * p[:, 1]) + 0.05 * np.sin(11.0 * p[:, 2] + 1.0) + 0.03 * np.sin(17.0 * p[:, 0] * p[:, 1])
    s.positions[:, :3] = (p * disp[:, None] * 0.5).astype(np.float32)
    return 1, s


def deformed(geo, phase):
    pos, att = geo.positions.copy(), geo.attributes.copy()
    p = pos[:, :3]
    pos[:, :3] = p * (np.float32(1.0) + np.float32(0.05) * np.sin(np.float32(7.0) * p[:, 1:2] + np.float32(3.0) * p[:, 0:1] + np.float32(phase)))
    att[:, 2:4] += np.float32(0.01 * phase)
    return pos, att


def numpy_normals(pos, att, idx):
    """Route (a): area-weighted smooth normals in numpy (float32; np.add.at sums in index order), octahedral-encoded into a copy of `att`."""
    p = pos[:, :3]
    tri = idx.reshape(-1, 3)
    c = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]).astype(np.float32)
    s = np.zeros_like(p)
    for k in range(3):
        np.add.at(s, tri[:, k], c)
    n = s / np.maximum(np.linalg.norm(s, axis=1, keepdims=True), np.float32(1e-30))
    e = n[:, 0:2] / np.maximum(np.abs(n).sum(axis=1, keepdims=True), np.float32(1e-30))
    low = n[:, 2] < 0
    f = (np.float32(1.0) - np.abs(e[:, ::-1])) * np.where(e >= 0, np.float32(1.0), np.float32(-1.0))
    out = att.copy()
    out[:, 0:2] = np.where(low[:, None], f, e)
    return out


def call_us(r, call, reps=20):
    """(median HIP-event microseconds between the call's first and last stream operation, median host microseconds of the call)"""
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e6)
        b.record(stream)
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return float(np.median(dev)), float(np.median(host))


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    for name in names:
        fs, rebuild = scene_of(name, orc)
        mesh, geo = mesh_of(name)
        inst = fs.get("instances")
        ids = np.flatnonzero(inst[:, 0] == mesh)
        mats = inst[ids, 5:21].view(np.float32).copy()
        shapes = [deformed(geo, k) for k in range(2)]
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        before = frame_ms(r, W, H, fs.num_lights)
        k = [0]
        def with_attrs():
            k[0] ^= 1; r.set_mesh_vertices(mesh, *shapes[k[0]])
        def positions_only():
            k[0] ^= 1; r.set_mesh_vertices(mesh, shapes[k[0]][0])
        full, full_host = call_us(r, with_attrs)
        posonly, pos_host = call_us(r, positions_only)
        moved, _ = call_us(r, lambda: r.set_instance_transforms(ids, mats))
        after = frame_ms(r, W, H, fs.num_lights)
        # the routes to correct normals / from device memory
        idx = np.asarray(geo.indices, np.uint32)
        dev = torch.device("cuda", r.device)
        tens = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in sh) for sh in shapes]
        def route_a():
            k[0] ^= 1; p, a = shapes[k[0]]; r.set_mesh_vertices(mesh, p, numpy_normals(p, a, idx))
        def route_b():
            k[0] ^= 1; r.set_mesh_vertices(mesh, shapes[k[0]][0], normals="recompute")
        def route_c():
            k[0] ^= 1; r.set_mesh_vertices(mesh, *tens[k[0]])
        def route_d():
            k[0] ^= 1; r.set_mesh_vertices(mesh, tens[k[0]][0], normals="recompute")
        routes = {}
        route_b(); r.sync()      # (the one-time adjacency build is not part of a call's steady cost)
        for key, fn in (("a_host_numpy_normals", route_a), ("b_host_recompute", route_b), ("c_device_keep", route_c), ("d_device_recompute", route_d)):
            us, host = call_us(r, fn)
            routes[key] = {"us": round(us, 1), "us_host": round(host, 1), "ms_frame_after": round(frame_ms(r, W, H, fs.num_lights), 3)}
        rejects = r.deform_rejects()
        t0 = time.perf_counter()
        fs2 = rebuild()
        r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE)
        r2.sync()
        rebuild_s = time.perf_counter() - t0
        print(json.dumps({"scene": name, "tris": int(fs.counts()["tris"]), "mesh_vertices": int(len(geo.positions)), "mesh_instances": int(len(ids)),
                          "tris_rewritten": int(inst[ids, 3].sum()), "upload_bytes": int(len(geo.positions)) * 64,
                          "us_with_attributes": round(full, 1), "us_host_with_attributes": round(full_host, 1),
                          "us_positions_only": round(posonly, 1), "us_host_positions_only": round(pos_host, 1),
                          "us_set_instance_transforms_same_instances": round(moved, 1),
                          "ms_frame_before": round(before, 3), "ms_frame_after": round(after, 3), "s_rebuild_and_recreate": round(rebuild_s, 3),
                          "routes": routes, "deform_rejects": rejects}), flush=True)
        del r, r2


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
