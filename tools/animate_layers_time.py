"""Cost of layering clips per frame (include/frt.h: frt_renderer_animate_layers; DESIGN.md section 11, "Layering clips"): the character of
tools/animate_blend_time.py (16 spheres of 162 vertices under a 64-joint skeleton and 8 morph targets, three clips with LINEAR translation,
rotation and scale channels on every joint and a weights channel), four masks over limbs of the skeleton. Routes, every one with
normals="recompute":
  (a2, a8) r.animate_layers(binding, layers) with two and with eight layers (override, additive and blend layers in turn, three in four under a
           mask): the layers folded in the rig kernel, then the batched pose
  (b2, b8) rig.evaluate_layers(layers, masks) on the host, then r.set_mesh_poses with the host arrays
  (c1)     r.animate(binding, clip, t): the single-clip call, whose kernel is the instantiation for a sample list
  (c2)     r.animate_blend(binding, samples) with two samples: the same instantiation
The single-clip and blend paths against the parent commit are (c1) here against tools/animate_blend_time.py's c1 and a2 there, run in turn on both
trees in one session (profiles/animation_layers.md).
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the
routes are timed in turn, three rounds, and the median of the rounds' medians is reported with the rounds beside it. One JSON line.
Usage: python tools/animate_layers_time.py"""
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
from animate_blend_time import skeleton, P, JOINTS, TARGETS, KEYS, CLIPS

F = np.float32
MODES = ("override", "additive", "blend")


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
    masks = np.stack([rig.mask(8), rig.mask(16, value=0.5), rig.mask([24, 32], value=0.75, base=0.25), rig.mask(4)])      # limbs, and the upper spine
    b = r.bind_rig(rig, ids)
    r.set_rig_masks(b, masks)
    r.animate(b, 0, 0.0); r.sync()      # (the one-time adjacency builds are not part of a call's steady cost)
    frame = [0]

    def now(k=0):
        return ((frame[0] + 7 * k) * 0.0137) % duration

    def layers(n):
        frame[0] += 1
        out = [(0, now(), 1.0)]
        for k in range(1, n):
            mode = MODES[(k - 1) % 3]
            out.append(frt.Layer(k % CLIPS, now(k), 0.25 + 0.1 * k if mode != "blend" else 0.5 * k, mask=None if k % 4 == 0 else (k - 1) % 4, mode=mode,
                                 reference=((k + 1) % CLIPS, 0.0) if mode == "additive" else None))
        return out

    def samples(n):
        frame[0] += 1
        return [(k % CLIPS, now(k), 0.25 + 0.5 * k) for k in range(n)]

    def single():
        frame[0] += 1
        return now()

    routes = [("a2_animate_layers", lambda: r.animate_layers(b, layers(2))), ("a8_animate_layers", lambda: r.animate_layers(b, layers(8))),
              ("b2_host_evaluate_layers_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_layers(layers(2), masks))),
              ("b8_host_evaluate_layers_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_layers(layers(8), masks))),
              ("c1_animate", lambda: r.animate(b, 0, single())), ("c2_animate_blend_of_two", lambda: r.animate_blend(b, samples(2)))]
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
                      "joints": JOINTS, "targets": TARGETS, "keys_per_channel": KEYS, "clips": CLIPS, "masks": int(masks.shape[0]), "routes": out,
                      "a8_and_b8_agree": agree, "deform_rejects": r.deform_rejects()}), flush=True)


if __name__ == "__main__":
    main()
