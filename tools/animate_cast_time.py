"""Cost of animating a cast per frame (include/frt.h: frt_renderer_animate_cast; DESIGN.md section 11, "Animating a cast"): the Cornell Box with C
copies of the 16-mesh character of tools/animate_time.py (16 spheres of 162 vertices, 64 joints, 8 morph targets, a binding per copy) and P prop rigs
of 9 small planes each (a 9-node rig of tools/animate_instances_time.py, a binding per prop), at (C, P) = (1, 1), (4, 4), (16, 16). Two routes to
the same replica, normals="recompute":
  (a) one r.animate_cast over all C + P bindings
  (b) the same entries as single calls: P times r.animate_instances, then C times r.animate
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it (for (b) that holds the wait
in which the first animate reads the matrices back after the animate_instances calls), medians of 20; the routes are timed in turn, three rounds
(a b a b a b), and the median of the rounds' medians is reported with the rounds beside it. Whether both routes end in the same triangle slots is
checked last. One JSON line per (C, P). A library without animate_cast (an earlier commit) times route (b) alone.
Usage: python tools/animate_cast_time.py [C,P ...]"""
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
from animate_time import skeleton, P as MESHES, JOINTS, TARGETS
from animate_instances_time import node_rig

F = np.float32
PROP = 9


def add_prop(r, k):
    """Nine small planes in a row; returns their instance ids and the matrices they were added with (the binding's offsets)."""
    mats = np.tile(np.eye(4, dtype=F).reshape(1, 16), (PROP, 1))
    mats[:, [0, 5, 10]] = F(0.03)
    mats[:, 12] = (np.arange(PROP, dtype=F) - F(4)) * F(0.08)
    mats[:, 13] = F(-0.9) + F(0.04) * F(k)
    first = r.add_instances([0] * PROP, [0] * PROP, mats)
    return np.arange(first, first + PROP), mats


def measure(orc, C, P):
    fs, _ = scene_of("cornell", orc)
    r = frt.Renderer(fs, 256, 144, flags=frt.FLAG_PIPELINE)      # (no frame is timed here)
    rs = torch.cuda.ExternalStream(r.stream_handle(0))
    rig, duration = skeleton()
    prop_rig, _ = node_rig(PROP)
    characters, props = [], []
    for c in range(C):
        ids, geo = add_character(r, MESHES)
        pos = np.ascontiguousarray(geo.positions, F)
        j, w = synthetic_skin(pos, JOINTS)
        deltas = (0.02 * (np.random.default_rng(MESHES).random((TARGETS, len(pos), 3)) - 0.5)).astype(F)
        for m in ids:
            r.set_mesh_morph_targets(m, deltas)
            r.set_mesh_skin(m, j, w, num_joints=JOINTS)
        characters.append(r.bind_rig(rig, ids))
    for k in range(P):
        ids, mats = add_prop(r, k)
        props.append(r.bind_rig_instances(prop_rig, ids, np.arange(PROP), offsets=mats))
    frame = [0]

    def now():
        frame[0] += 1
        return (frame[0] * 0.0137) % duration

    def route_a():
        t = now()
        r.animate_cast([(b, 0, t) for b in props + characters])

    def route_b():
        t = now()
        for b in props:
            r.animate_instances(b, 0, t)
        for b in characters:
            r.animate(b, 0, t)

    routes = [("b_single_calls", route_b)]
    if hasattr(r, "animate_cast"):
        routes.insert(0, ("a_animate_cast", route_a))
    for _, fn in routes:      # (the one-time adjacency builds and device tables are not part of a call's steady cost)
        fn(); r.sync()
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
    print(json.dumps({"scene": "cornell", "characters": C, "props": P, "bindings": C + P, "meshes_posed": C * MESHES, "instances_moved": P * PROP,
                      "scene_triangles": int(c["tris"]), "routes": out, "routes_agree": len(set(slots)) == 1,
                      "transform_rejects": r.transform_rejects(), "deform_rejects": r.deform_rejects()}), flush=True)


def main(args):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    for arg in args or ["1,1", "4,4", "16,16"]:
        C, P = (int(x) for x in arg.split(","))
        measure(orc, C, P)


if __name__ == "__main__":
    main(sys.argv[1:])
