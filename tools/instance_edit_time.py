"""Cost of adding and removing an instance on the device (include/frt.h: frt_renderer_add_instances, _remove_instances) on the
Cornell Box, the 82k-triangle blob and the 246k-triangle colonnade (tests/_scenes.py): microseconds per call (HIP events on the renderer's stream
around the call, median of 20) for one more instance of the largest instance's mesh and for taking it out again, in both rebuild modes; the frame
time (1920x1080, 8 bounces, FLAG_PIPELINE) before the edits, with the added instance in place and of a renderer over the equivalent fresh host build;
and the host path the calls replace (SceneBuilder.add_instances = a host build, plus a new Renderer). One JSON line per scene.
Usage: python tools/instance_edit_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of, frame_ms


def event_us(r, call):
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    for name in names:
        fs, rebuild = scene_of(name, orc)
        inst = fs.get("instances")
        biggest = int(np.argmax(inst[:, 3]))
        mesh, mat = int(inst[biggest, 0]), int(inst[biggest, 1])
        m = inst[biggest, 5:21].view(np.float32).copy()
        m[12:15] += np.float32(0.05)                                     # beside the original, overlapping it: the tree has real work to do
        n = len(inst)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        rec = {"scene": name, "tris": int(fs.counts()["tris"]), "instances": n, "one_instance_tris": int(inst[biggest, 3])}
        rec["ms_frame_before"] = round(frame_ms(r, W, H, fs.num_lights), 3)
        for quality in ("morton", "sah"):
            add, rem = [], []
            r.add_instances(mesh, mat, m, quality=quality); r.remove_instances(n, quality=quality)      # (the first call allocates and grows)
            for _ in range(20):
                add.append(event_us(r, lambda: r.add_instances(mesh, mat, m, quality=quality)))
                rem.append(event_us(r, lambda: r.remove_instances(n, quality=quality)))
            rec[f"us_add_{quality}"] = round(float(np.median(add)), 1)
            rec[f"us_remove_{quality}"] = round(float(np.median(rem)), 1)
            r.add_instances(mesh, mat, m, quality=quality)
            rec[f"ms_frame_after_add_{quality}"] = round(frame_ms(r, W, H, fs.num_lights), 3)
            r.remove_instances(n, quality=quality)
        t0 = time.perf_counter()
        fs2 = rebuild()
        t1 = time.perf_counter()
        fs2.add_instances(mesh, mat, m)
        t2 = time.perf_counter()
        r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE)
        r2.sync()
        t3 = time.perf_counter()
        rec["ms_frame_fresh_host_build"] = round(frame_ms(r2, W, H, fs2.num_lights), 3)
        rec["s_host_add_instances"] = round(t2 - t1, 3)
        rec["s_host_build_and_recreate"] = round((t1 - t0) + (t3 - t2), 3)
        print(json.dumps(rec), flush=True)
        del r, r2


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
