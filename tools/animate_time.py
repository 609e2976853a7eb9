"""Cost of animating a character per frame (include/frt.h: frt_renderer_animate; DESIGN.md section 11, "Animation"): the 16-mesh character of
tools/pose_batch_time.py (16 spheres of 162 vertices, one instance each, added to the Cornell Box) under a 64-joint skeleton (a chain of 8 spines
with 7 limbs of 8 joints) and 8 morph targets, one clip with LINEAR translation, rotation and scale channels on every joint and a weights channel.
Three routes to the same posed replica, every one with normals="recompute":
  (a) r.animate(binding, clip, t): one kernel evaluates the clip on the device, then the batched pose from the renderer's own buffers
  (b) rig.evaluate(clip, t) on the host, then r.set_mesh_poses with the host arrays: the route there was before
  (c) as (b), the palette and the weights uploaded as torch tensors first, then r.set_mesh_poses with the tensors
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the routes
are timed in turn, three rounds (a b c a b c a b c), and the median of the rounds' medians is reported with the rounds beside it. Whether the three
routes end in the same triangle slots is checked last. One JSON line. Usage: python tools/animate_time.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from skin_time import synthetic_skin, call_us
from pose_batch_time import add_character

F = np.float32
P, JOINTS, TARGETS, KEYS = 16, 64, 8, 32


def skeleton():
    """(frt.Rig, duration): 64 nodes, every one a joint, near the identity; 32 keys per channel over one second."""
    rng = np.random.default_rng(64)
    par = np.full(JOINTS, -1, np.int32)
    par[1:8] = np.arange(0, 7)                                  # the spine
    for limb in range(7):
        first = 8 + 8 * limb
        par[first] = 1 + limb
        par[first + 1:first + 8] = np.arange(first, first + 7)
    times = np.linspace(0.0, 1.0, KEYS).astype(F)

    def quats(n):
        q = np.tile(F([0, 0, 0, 1]), (n, 1)) + F(0.02) * rng.standard_normal((n, 4)).astype(F)
        return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)

    channels = []
    for n in range(JOINTS):
        channels += [{"node": n, "path": "translation", "interpolation": "LINEAR", "times": times, "values": (0.002 * rng.standard_normal((KEYS, 3))).astype(F)},
                     {"node": n, "path": "rotation", "interpolation": "LINEAR", "times": times, "values": quats(KEYS)},
                     {"node": n, "path": "scale", "interpolation": "LINEAR", "times": times, "values": (1.0 + 0.01 * rng.standard_normal((KEYS, 3))).astype(F)}]
    channels.append({"path": "weights", "interpolation": "LINEAR", "times": times, "values": rng.uniform(0.0, 1.0, (KEYS, TARGETS)).astype(F)})
    return frt.Rig(par, translations=(0.002 * rng.standard_normal((JOINTS, 3))).astype(F), rotations=quats(JOINTS), joint_nodes=np.arange(JOINTS),
                   num_targets=TARGETS, clips=[("idle", channels)]), 1.0


def main():
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    fs, _ = scene_of("cornell", orc)
    r = frt.Renderer(fs, 256, 144, flags=frt.FLAG_PIPELINE)      # (no frame is timed here)
    dev = torch.device("cuda", r.device)
    rs = torch.cuda.ExternalStream(r.stream_handle(0))
    ids, geo = add_character(r, P)
    pos = np.ascontiguousarray(geo.positions, F)
    j, w = synthetic_skin(pos, JOINTS)
    deltas = (0.02 * (np.random.default_rng(P).random((TARGETS, len(pos), 3)) - 0.5)).astype(F)
    for m in ids:
        r.set_mesh_morph_targets(m, deltas)
        r.set_mesh_skin(m, j, w, num_joints=JOINTS)
    rig, duration = skeleton()
    b = r.bind_rig(rig, ids)
    r.animate(b, 0, 0.0); r.sync()      # (the one-time adjacency builds are not part of a call's steady cost)
    frame = [0]

    def now():
        frame[0] += 1
        return (frame[0] * 0.0137) % duration

    def route_a():
        r.animate(b, 0, now())

    def route_b():
        r.set_mesh_poses(ids, *rig.evaluate(0, now()))

    def route_c():
        pal, wt = rig.evaluate(0, now())
        r.set_mesh_poses(ids, torch.from_numpy(pal).to(dev), torch.from_numpy(wt).to(dev))

    routes = (("a_animate", route_a), ("b_host_evaluate_then_host_arrays", route_b), ("c_host_evaluate_then_tensors", route_c))
    rounds = {k: [] for k, _ in routes}
    for _ in range(3):
        for key, fn in routes:
            fn(); r.sync()
            rounds[key].append(call_us(rs, rs, fn, r.sync))
    out = {k: {"us": float(np.median([x[0] for x in v])), "us_host": float(np.median([x[1] for x in v])), "rounds": v} for k, v in rounds.items()}
    slots = []
    for _, fn in routes:
        frame[0] = 40
        fn()
        slots.append(r.read_scene("tri_slots").tobytes())
    c = r.scene_counts()
    print(json.dumps({"scene": "cornell", "meshes": P, "vertices": int(P * len(pos)), "scene_triangles": int(c["tris"]), "joints": JOINTS, "targets": TARGETS,
                      "keys_per_channel": KEYS, "routes": out, "routes_agree": slots[0] == slots[1] == slots[2], "deform_rejects": r.deform_rejects()}), flush=True)


if __name__ == "__main__":
    main()
