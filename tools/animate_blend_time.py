"""Cost of blending clips per frame (include/frt.h: frt_renderer_animate_blend; DESIGN.md section 11, "Blending clips"): the character of
tools/animate_time.py (16 spheres of 162 vertices under a 64-joint skeleton and 8 morph targets) with three clips instead of one, every clip with
LINEAR translation, rotation and scale channels on every joint and a weights channel. Routes, every one with normals="recompute":
  (a2, a8) r.animate_blend(binding, samples) with two and with eight samples: the clips blended in the rig kernel, then the batched pose
  (b2, b8) rig.evaluate_blend(samples) on the host, then r.set_mesh_poses with the host arrays
  (c1)     r.animate(binding, clip, t): the single-clip call, which runs the same kernel with a list of one
  (c2)     r.animate_cast([(binding, clip, t)]): the single-clip cast of one entry
The single-clip path against the parent commit is tools/animate_time.py and tools/animate_cast_time.py, which both commits have, run in turn on
both trees in one session (profiles/animation_blend.md).
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the
routes are timed in turn, three rounds, and the median of the rounds' medians is reported with the rounds beside it. One JSON line.
Usage: python tools/animate_blend_time.py"""
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
P, JOINTS, TARGETS, KEYS, CLIPS = 16, 64, 8, 32, 3


def skeleton():
    """(frt.Rig, duration): tools/animate_time.py's skeleton with CLIPS clips, each with its own keys."""
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

    clips = []
    for c in range(CLIPS):
        channels = []
        for n in range(JOINTS):
            channels += [{"node": n, "path": "translation", "interpolation": "LINEAR", "times": times, "values": (0.002 * rng.standard_normal((KEYS, 3))).astype(F)},
                         {"node": n, "path": "rotation", "interpolation": "LINEAR", "times": times, "values": quats(KEYS)},
                         {"node": n, "path": "scale", "interpolation": "LINEAR", "times": times, "values": (1.0 + 0.01 * rng.standard_normal((KEYS, 3))).astype(F)}]
        channels.append({"path": "weights", "interpolation": "LINEAR", "times": times, "values": rng.uniform(0.0, 1.0, (KEYS, TARGETS)).astype(F)})
        clips.append((f"clip{c}", channels))
    return frt.Rig(par, translations=(0.002 * rng.standard_normal((JOINTS, 3))).astype(F), rotations=quats(JOINTS), joint_nodes=np.arange(JOINTS),
                   num_targets=TARGETS, clips=clips), 1.0


def main():
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    fs, _ = scene_of("cornell", orc)
    r = frt.Renderer(fs, 256, 144, flags=frt.FLAG_PIPELINE)      # (no frame is timed here)
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

    def now(k=0):
        return ((frame[0] + 7 * k) * 0.0137) % duration

    def samples(n):
        frame[0] += 1
        return [(k % CLIPS, now(k), 0.25 + 0.5 * k) for k in range(n)]

    def single():
        frame[0] += 1
        return now()

    routes = [("a2_animate_blend", lambda: r.animate_blend(b, samples(2))), ("a8_animate_blend", lambda: r.animate_blend(b, samples(8))),
              ("b2_host_evaluate_blend_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_blend(samples(2)))),
              ("b8_host_evaluate_blend_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_blend(samples(8)))),
              ("c1_animate", lambda: r.animate(b, 0, single())), ("c2_animate_cast_of_one", lambda: r.animate_cast([(b, 0, single())]))]
    rounds = {k: [] for k, _ in routes}
    for _ in range(3):
        for key, fn in routes:
            fn(); r.sync()
            rounds[key].append(call_us(rs, rs, fn, r.sync))
    out = {k: {"us": float(np.median([x[0] for x in v])), "us_host": float(np.median([x[1] for x in v])), "rounds": v} for k, v in rounds.items()}
    slots = []
    for fn in (routes[1][1], routes[3][1]):
        frame[0] = 40
        fn()
        slots.append(r.read_scene("tri_slots").tobytes())
    agree = slots[0] == slots[1]
    c = r.scene_counts()
    print(json.dumps({"scene": "cornell", "meshes": P, "vertices": int(P * len(pos)), "scene_triangles": int(c["tris"]),
                      "joints": JOINTS, "targets": TARGETS, "keys_per_channel": KEYS, "clips": CLIPS, "routes": out, "a8_and_b8_agree": agree,
                      "deform_rejects": r.deform_rejects()}), flush=True)


if __name__ == "__main__":
    main()
