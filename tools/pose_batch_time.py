"""Cost of posing a character of P meshes (include/frt.h: frt_renderer_set_mesh_poses; DESIGN.md section 11, "Posing several meshes"): P sphere meshes
(162 vertices, 320 triangles each, one instance each) that share one synthetic skin layout of 64 joints and four morph targets, added to the Cornell
Box and to the colonnade through add_meshes / add_instances (so the replica's tree is the device-built one), for P in 1, 4, 16, 64. Four routes, every
one with normals="recompute", microseconds per posed character (HIP events on the renderer's stream around the whole route, median of 20; the route's
host part beside it):
  (a) the loop of P set_mesh_pose calls, each a batch of one mesh
  (b) one set_mesh_poses from a host palette
  (c) one set_mesh_poses from a device palette
  (d) one set_mesh_poses with morph weights as well (morph, then skin; host inputs)
and whether (a) and (b) end in the same triangle slots. One JSON line per scene and P. Usage: python tools/pose_batch_time.py [cornell colonnade]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from skin_time import synthetic_skin, palettes, call_us

F = np.float32
JOINTS, TARGETS = 64, 4


def add_character(r, P):
    """P spheres in a row, each a mesh of its own with one instance; returns their mesh ids and the geometry."""
    geo = frt.geometry.create_sphere(2)
    first = r.add_meshes([geo] * P)
    ids = list(range(first, first + P))
    mats = np.tile(np.eye(4, dtype=F).reshape(1, 16), (P, 1))
    mats[:, [0, 5, 10]] = F(0.05)
    mats[:, 12] = (np.arange(P, dtype=F) - F(P - 1) / 2) * F(0.9 / max(P, 8))
    mats[:, 13] = F(-0.2)
    r.add_instances(ids, [0] * P, mats)
    return ids, geo


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 256, 144      # (no frame is timed here)
    for name in names:
        for P in (1, 4, 16, 64):
            fs, _ = scene_of(name, orc)
            r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
            dev = torch.device("cuda", r.device)
            rs = torch.cuda.ExternalStream(r.stream_handle(0))
            ids, geo = add_character(r, P)
            pos = np.ascontiguousarray(geo.positions, F)
            j, w = synthetic_skin(pos, JOINTS)
            rng = np.random.default_rng(P)
            deltas = (0.02 * (rng.random((TARGETS, len(pos), 3)) - 0.5)).astype(F)
            for m in ids:
                r.set_mesh_morph_targets(m, deltas)
                r.set_mesh_skin(m, j, w, num_joints=JOINTS)
            pals = palettes(JOINTS)
            d_pals = [torch.from_numpy(m).to(dev) for m in pals]
            wts = [np.linspace(0.1, 0.9, TARGETS).astype(F), np.linspace(0.9, 0.1, TARGETS).astype(F)]
            r.set_mesh_poses(ids, pals[0]); r.sync()      # (the one-time adjacency builds are not part of a call's steady cost)
            k = [0]
            def route_a():
                k[0] ^= 1
                for m in ids:
                    r.set_mesh_pose(m, pals[k[0]])
            def route_b():
                k[0] ^= 1; r.set_mesh_poses(ids, pals[k[0]])
            def route_c():
                k[0] ^= 1; r.set_mesh_poses(ids, d_pals[k[0]])
            def route_d():
                k[0] ^= 1; r.set_mesh_poses(ids, pals[k[0]], wts[k[0]])
            routes = {}
            for key, fn in (("a_loop_of_set_mesh_pose", route_a), ("b_set_mesh_poses_host", route_b), ("c_set_mesh_poses_device", route_c),
                            ("d_set_mesh_poses_morph_and_skin_host", route_d)):
                fn(); r.sync()
                us, host = call_us(rs, rs, fn, r.sync)
                routes[key] = {"us": us, "us_host": host}
            route_a(); want = r.read_scene("tri_slots").tobytes()
            k[0] ^= 1; route_b(); same = r.read_scene("tri_slots").tobytes() == want
            c = r.scene_counts()
            print(json.dumps({"scene": name, "meshes": P, "vertices": int(P * len(pos)), "triangles_posed": int(P * len(geo.indices) // 3), "scene_triangles": int(c["tris"]),
                              "joints": JOINTS, "targets": TARGETS, "routes": routes, "a_and_b_agree": bool(same), "deform_rejects": r.deform_rejects()}), flush=True)
            del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "colonnade"])
