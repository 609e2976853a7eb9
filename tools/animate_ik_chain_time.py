"""Cost of chain IK per frame (include/frt.h: FRT_GOAL_CHAIN; DESIGN.md section 11, "Chain IK"), in the manner of tools/animate_ik_time.py: its
character (16 spheres of 162 vertices, 64 joints, 8 morph targets, three clips, four masks) and its two-layer stack, on a 64-joint skeleton whose
spine is 32 nodes long (the skeleton of animate_blend_time.py has no path of more than 16 nodes, and a chain of 31 bones needs one of 32), four
limbs of 8 nodes on it. Routes, every one with normals="recompute":
  (g0)          r.animate_layers(binding, layers) on a binding without goals: the instantiation without goal code
  (g2)          two two-bone goals: the goal instantiation without chain code
  (cB_sS)       one chain goal of B = 4, 8, 31 bones at S = 1, 8, 16 sweeps: r.set_rig_goal_targets(binding, host row), then r.animate_layers: the chain
                instantiation of the rig kernel (one round of two barriers, S B steps in wave lanes), then the batched pose
  (h0, hB_sS)   rig.evaluate_layers(layers, masks[, goals, targets]) on the host, then r.set_mesh_poses with the host arrays, for the same nine goals
The parent's rows (no goals, two two-bone goals on the standard skeleton) are re-measured by tools/animate_ik_time.py, which both commits have, run
in turn on both trees in one session (profiles/animation_ik_chain.md).
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the
routes are timed in turn, three rounds, and the median of the rounds' medians is reported with the rounds beside it. One JSON line.
Usage: python tools/animate_ik_chain_time.py"""
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
from animate_blend_time import P, JOINTS, TARGETS, KEYS, CLIPS

F = np.float32
SPINE = 32
BONES, SWEEPS = (4, 8, 31), (1, 8, 16)
HOST = tuple((b, s) for b in BONES for s in SWEEPS)


def deep_skeleton():
    """(frt.Rig, duration): animate_blend_time.skeleton's values on a hierarchy with a spine of 32 nodes (0 .. 31) and four limbs of 8 nodes on
    spine nodes 7, 15, 23 and 31."""
    rng = np.random.default_rng(64)
    par = np.full(JOINTS, -1, np.int32)
    par[1:SPINE] = np.arange(0, SPINE - 1)
    for limb in range(4):
        first = SPINE + 8 * limb
        par[first] = 7 + 8 * limb
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
    rig, duration = deep_skeleton()
    masks = np.stack([rig.mask(8), rig.mask(16, value=0.5), rig.mask([24, 32], value=0.75, base=0.25), rig.mask(4)])
    sets = {"g0": [], "g2": [frt.TwoBone(32, 35, 39), frt.TwoBone(40, 43, 47)]}
    for b in BONES:
        for s in SWEEPS:
            sets[f"c{b}_s{s}"] = [frt.Chain(0, b, sweeps=s)]      # the spine's first b bones: the limbs and the rest of the spine hang off it
    bind = {}
    for key, goals in sets.items():      # one binding a goal set: no route changes another's state
        bind[key] = r.bind_rig(rig, ids)
        r.set_rig_masks(bind[key], masks)
        r.set_rig_goals(bind[key], goals or None)
    r.animate(bind["g0"], 0, 0.0); r.sync()      # (the one-time adjacency builds are not part of a call's steady cost)
    frame = [0]

    def layers():
        frame[0] += 1
        t = (frame[0] * 0.0137) % duration
        return [(0, t, 1.0), frt.Layer(1, (t + 0.1) % duration, 0.35, mask=0, mode="override")]

    def rows(n):
        """Targets that move a little every frame, near the skeleton (its bones are a few thousandths long), at half weight."""
        rng = np.random.default_rng(frame[0])
        t = np.zeros((n, 8), F)
        t[:, :3] = 0.01 * rng.standard_normal((n, 3))
        t[:, 3] = 0.5
        return t

    def device(key):
        def fn():
            stack = layers()      # (the frame advances here; the rows are this frame's)
            if sets[key]:
                r.set_rig_goal_targets(bind[key], rows(len(sets[key])))
            r.animate_layers(bind[key], stack)
        return fn

    def host(key):
        def fn():
            stack = layers()
            goals = sets[key]
            r.set_mesh_poses(ids, *(rig.evaluate_layers(stack, masks, goals, rows(len(goals))) if goals else rig.evaluate_layers(stack, masks)))
        return fn

    routes = [(key, device(key)) for key in sets] + [("h0", host("g0"))] + [(f"h{b}_s{s}", host(f"c{b}_s{s}")) for b, s in HOST]
    rounds = {k: [] for k, _ in routes}
    for _ in range(3):
        for key, fn in routes:
            fn(); r.sync()
            rounds[key].append(call_us(rs, rs, fn, r.sync))
    out = {k: {"us": float(np.median([x[0] for x in v])), "us_host": float(np.median([x[1] for x in v])), "rounds": v} for k, v in rounds.items()}
    slots = []
    for fn in (device("c31_s16"), host("c31_s16")):      # the device route and the host route leave the same replica
        frame[0] = 40
        fn()
        slots.append(r.read_scene("tri_slots").tobytes())
    frame[0] = 40
    plain = rig.evaluate_layers(layers(), masks)[0]
    frame[0] = 40
    moved = float(np.abs(rig.evaluate_layers(layers(), masks, sets["c31_s16"], rows(1))[0] - plain).max())
    c = r.scene_counts()
    print(json.dumps({"scene": "cornell", "meshes": P, "vertices": int(P * len(pos)), "scene_triangles": int(c["tris"]), "joints": JOINTS, "spine_nodes": SPINE, "targets": TARGETS,
                      "keys_per_channel": KEYS, "clips": CLIPS, "masks": int(masks.shape[0]), "layers": 2, "routes": out, "c31_s16_and_its_host_route_agree": slots[0] == slots[1],
                      "largest_palette_change_by_c31_s16": moved, "deform_rejects": r.deform_rejects()}), flush=True)


if __name__ == "__main__":
    main()
