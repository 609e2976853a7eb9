"""Cost of moving instances (include/frt.h: frt_renderer_set_instance_transforms) on the Cornell Box, the 82k-triangle blob and
the 246k-triangle colonnade (tests/_scenes.py): microseconds per call for one instance and for all of them (HIP events on the renderer's stream,
median of 20), the frame time before and after a move (1920x1080, two-stream schedule), and the host rebuild + renderer re-create it replaces.
One JSON line per scene. Usage: python tools/instance_update_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle


def scene_of(name, orc):
    import _scenes
    if name == "cornell":
        return frt.scenes.create_cornell_box(), lambda: frt.scenes.create_cornell_box()
    if name == "blob":
        return _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)[0], lambda: _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)[0]
    return _scenes.colonnade(frt, orc)[0], lambda: _scenes.colonnade(frt, orc)[0]


def frame_ms(r, W, H, nl, frames=24):
    cams = [frt.CameraController().build_uniform(W / H, f, nl) for f in range(frames + 4)]
    r.clear()
    for c in cams[:4]: r.render(c)
    r.sync(); t0 = time.perf_counter()
    for c in cams[4:]: r.render(c)
    r.sync()
    return (time.perf_counter() - t0) / frames * 1e3


def call_us(r, ids, mats, reps=20):
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        r.set_instance_transforms(ids, mats)
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    for name in names:
        fs, rebuild = scene_of(name, orc)
        inst = fs.get("instances")
        n = len(inst)
        cur = inst[:, 5:21].view(np.float32).copy()
        moved = cur.copy(); moved[:, 12] += np.float32(0.01)          # every instance 1 cm along x
        biggest = int(np.argmax(inst[:, 3]))
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        before = frame_ms(r, W, H, fs.num_lights)
        one = call_us(r, [biggest], moved[biggest:biggest + 1])
        every = call_us(r, np.arange(n), moved)
        after = frame_ms(r, W, H, fs.num_lights)
        t0 = time.perf_counter()
        fs2 = rebuild()
        r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE)
        r2.sync()
        rebuild_s = time.perf_counter() - t0
        print(json.dumps({"scene": name, "tris": int(fs.counts()["tris"]), "instances": n, "us_one_instance": round(one, 1), "one_instance_tris": int(inst[biggest, 3]),
                          "us_all_instances": round(every, 1), "ms_frame_before": round(before, 3), "ms_frame_after": round(after, 3),
                          "s_rebuild_and_recreate": round(rebuild_s, 3)}), flush=True)
        del r, r2


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
