"""Cost of node animation per frame (include/frt.h: frt_renderer_animate_instances; DESIGN.md section 11, "Node animation"): every instance of the
colonnade (99 instances, tests/_scenes.py) and of the Cornell Box (9) hangs on a node of its own in a rig of as many nodes (a 4-ary tree near the
identity, LINEAR translation, rotation and scale channels of 32 keys on every node); the instance's matrix at creation is its offset, so it stays
about where it was. Two routes to the same replica:
  (a) r.animate_instances(binding, clip, t): one kernel evaluates the clip on the device, then the device-input instance transform from the binding's buffers
  (b) rig.evaluate_nodes(clip, t, ...) on the host, then r.set_instance_transforms with the host arrays
Per route: HIP-event microseconds on the renderer's stream around the whole route and the host's microseconds inside it, medians of 20; the routes are
timed in turn, three rounds (a b a b a b), and the median of the rounds' medians is reported with the rounds beside it. Whether both routes end in the
same triangle slots is checked last. One JSON line per scene. Usage: python tools/animate_instances_time.py [cornell colonnade]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from skin_time import call_us

F = np.float32
KEYS = 32


def node_rig(n):
    """(frt.Rig, duration): n nodes, node k under node (k - 1) // 4, near the identity; 32 keys per channel over one second."""
    rng = np.random.default_rng(n)
    par = np.array([-1] + [(k - 1) // 4 for k in range(1, n)], np.int32)
    times = np.linspace(0.0, 1.0, KEYS).astype(F)

    def quats(k):
        q = np.tile(F([0, 0, 0, 1]), (k, 1)) + F(0.01) * rng.standard_normal((k, 4)).astype(F)
        return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)

    channels = []
    for k in range(n):
        channels += [{"node": k, "path": "translation", "interpolation": "LINEAR", "times": times, "values": (0.002 * rng.standard_normal((KEYS, 3))).astype(F)},
                     {"node": k, "path": "rotation", "interpolation": "LINEAR", "times": times, "values": quats(KEYS)},
                     {"node": k, "path": "scale", "interpolation": "LINEAR", "times": times, "values": (1.0 + 0.01 * rng.standard_normal((KEYS, 3))).astype(F)}]
    return frt.Rig(par, clips=[("run", channels)], nodes_only=True), 1.0


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    for name in names:
        fs, _ = scene_of(name, orc)
        r = frt.Renderer(fs, 256, 144, flags=frt.FLAG_PIPELINE)      # (no frame is timed here)
        rs = torch.cuda.ExternalStream(r.stream_handle(0))
        n = fs.counts()["instances"]
        ids, nodes = np.arange(n), np.arange(n)
        offsets = fs.get("instances")[:, 5:21].view(F).copy()
        rig, duration = node_rig(n)
        b = r.bind_rig_instances(rig, ids, nodes, offsets=offsets)
        r.animate_instances(b, 0, 0.0); r.sync()      # (the tables of the device-input transform are made by the first call)
        frame = [0]

        def now():
            frame[0] += 1
            return (frame[0] * 0.0137) % duration

        def route_a():
            r.animate_instances(b, 0, now())

        def route_b():
            r.set_instance_transforms(ids, rig.evaluate_nodes(0, now(), nodes, offsets=offsets))

        routes = (("a_animate_instances", route_a), ("b_host_evaluate_nodes_then_host_arrays", route_b))
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
        print(json.dumps({"scene": name, "instances": int(n), "nodes": int(n), "scene_triangles": int(r.scene_counts()["tris"]), "keys_per_channel": KEYS, "routes": out,
                          "routes_agree": slots[0] == slots[1], "transform_rejects": r.transform_rejects()}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "colonnade"])
