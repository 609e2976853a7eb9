"""Cost of inverse kinematics per frame (include/frt.h: frt_renderer_set_rig_goals, _set_rig_goal_targets; DESIGN.md section 11, "Inverse
kinematics"): the character of tools/animate_layers_time.py (16 spheres of 162 vertices under a 64-joint skeleton and 8 morph targets, three clips,
four masks), a two-layer stack, and goals on the skeleton's seven limbs (a two-bone goal over each limb, an aim on each limb's tip, and one of each
on the spine: 16 in all). Routes, every one with normals="recompute":
  (g0)       r.animate_layers(binding, layers) on a binding without goals: the instantiation without goal code
  (g2, g16)  r.set_rig_goal_targets(binding, host rows) then r.animate_layers(binding, layers) with 2 and with 16 goals: one staged copy of
             32 bytes a goal, then the goal instantiation of the rig kernel (one round of two barriers a goal), then the batched pose
  (d16)      the same with the 16 targets in a device tensor: one device-to-device copy, nothing staged
  (h0, h16)  rig.evaluate_layers(layers, masks[, goals, targets]) on the host, then r.set_mesh_poses with the host arrays
The existing calls against the parent commit are measured by tools/animate_blend_time.py and tools/animate_layers_time.py, which both commits
have, run in turn on both trees in one session (profiles/animation_ik.md).
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the
routes are timed in turn, three rounds, and the median of the rounds' medians is reported with the rounds beside it. One JSON line.
Usage: python tools/animate_ik_time.py"""
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


def limb_goals():
    """16 goals: a two-bone goal and a tip aim on each of the seven limbs (nodes 8 + 8 l .. 15 + 8 l) and on the spine (nodes 0 .. 7)."""
    chains = [(8 + 8 * l, 11 + 8 * l, 15 + 8 * l) for l in range(7)] + [(0, 3, 7)]
    return [frt.TwoBone(*c) for c in chains] + [frt.Aim(c[2], (0.0, 1.0, 0.0)) for c in chains]


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
    masks = np.stack([rig.mask(8), rig.mask(16, value=0.5), rig.mask([24, 32], value=0.75, base=0.25), rig.mask(4)])
    every = limb_goals()
    sets = {0: [], 2: [every[0], every[8]], 16: every}      # 2: one limb's two-bone goal and the aim on its tip
    bind = {}
    for n, goals in sets.items():      # one binding a goal count: no route changes another's state
        bind[n] = r.bind_rig(rig, ids)
        r.set_rig_masks(bind[n], masks)
        r.set_rig_goals(bind[n], goals or None)
    r.animate(bind[0], 0, 0.0); r.sync()      # (the one-time adjacency builds are not part of a call's steady cost)
    frame = [0]

    def layers():
        frame[0] += 1
        t = (frame[0] * 0.0137) % duration
        return [(0, t, 1.0), frt.Layer(1, (t + 0.1) % duration, 0.35, mask=0, mode="override")]

    def rows(n):
        """Targets that move a little every frame, near the skeleton (its bones are a few hundredths long), at half weight; a pole on the limbs."""
        rng = np.random.default_rng(frame[0])
        t = np.zeros((n, 8), F)
        t[:, :3] = 0.05 * rng.standard_normal((n, 3))
        t[:, 3] = 0.5
        for k, g in enumerate(sets[n]):
            if isinstance(g, frt.TwoBone):
                t[k, 4:7], t[k, 7] = 0.05 * rng.standard_normal(3), 1.0
        return t

    dev_rows = torch.from_numpy(rows(16)).to(f"cuda:{r.device}")

    def device_targets():
        r.set_rig_goal_targets(bind[16], dev_rows)
        r.animate_layers(bind[16], layers())

    def with_goals(n):
        def fn():
            stack = layers()      # (the frame advances here; the rows are this frame's)
            r.set_rig_goal_targets(bind[n], rows(n))
            r.animate_layers(bind[n], stack)
        return fn

    routes = [("g0_animate_layers_without_goals", lambda: r.animate_layers(bind[0], layers())), ("g2_targets_then_animate_layers", with_goals(2)),
              ("g16_targets_then_animate_layers", with_goals(16)), ("d16_device_targets_then_animate_layers", device_targets),
              ("h0_host_evaluate_layers_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_layers(layers(), masks))),
              ("h16_host_evaluate_layers_ik_then_host_arrays", lambda: r.set_mesh_poses(ids, *rig.evaluate_layers(layers(), masks, sets[16], rows(16))))]
    rounds = {k: [] for k, _ in routes}
    for _ in range(3):
        for key, fn in routes:
            fn(); r.sync()
            rounds[key].append(call_us(rs, rs, fn, r.sync))
    out = {k: {"us": float(np.median([x[0] for x in v])), "us_host": float(np.median([x[1] for x in v])), "rounds": v} for k, v in rounds.items()}
    slots = []
    for fn in (routes[2][1], routes[5][1]):      # the device route and the host route leave the same replica
        frame[0] = 40
        fn()
        slots.append(r.read_scene("tri_slots").tobytes())
    frame[0] = 40
    plain = rig.evaluate_layers(layers(), masks)[0]
    frame[0] = 40
    moved = float(np.abs(rig.evaluate_layers(layers(), masks, sets[16], rows(16))[0] - plain).max())
    c = r.scene_counts()
    print(json.dumps({"scene": "cornell", "meshes": P, "vertices": int(P * len(pos)), "scene_triangles": int(c["tris"]), "joints": JOINTS, "targets": TARGETS,
                      "keys_per_channel": KEYS, "clips": CLIPS, "masks": int(masks.shape[0]), "layers": 2, "routes": out, "g16_and_h16_agree": slots[0] == slots[1],
                      "largest_palette_change_by_16_goals": moved, "deform_rejects": r.deform_rejects()}), flush=True)


if __name__ == "__main__":
    main()
