"""Cost of moving instances whose matrices live in a torch tensor on the GPU (include/frt.h: frt_renderer_set_instance_transforms_ex, FRT_TRANSFORM_DEVICE;
DESIGN.md section 11, "Transforms from device memory"): the host-array call — with the caller's device-to-host copy of the matrices in front of it, which
is what the device form removes — against the device-tensor call. Per case the median of 20 of two clocks: HIP events on the renderer's stream around the
call (what the stream sees, idle time while the host works included) and the host's wall clock from the start of the call until the stream has passed it.
Cases: the Cornell Box and the 246k-triangle colonnade of 99 instances (tests/_scenes.py), one instance (the largest) and all of them.
One JSON line per case. Usage: python tools/instance_update_device_time.py [cornell colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle


def timed(r, call, reps=20):
    """Median (event microseconds, wall microseconds) of `call`, after two calls that are not counted (tables, staging blocks, torch's allocator)."""
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    ev, wall = [], []
    for k in range(reps + 2):
        r.sync()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        t1 = time.perf_counter()
        if k >= 2:
            ev.append(a.elapsed_time(b) * 1e3); wall.append((t1 - t0) * 1e6)
    return round(float(np.median(ev)), 1), round(float(np.median(wall)), 1)


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    dev = torch.device("cuda", 0)
    for name in names:
        import _scenes
        fs = frt.scenes.create_cornell_box() if name == "cornell" else _scenes.colonnade(frt, orc)[0]
        inst = fs.get("instances")
        n = len(inst)
        moved = inst[:, 5:21].view(np.float32).copy(); moved[:, 12] += np.float32(0.01)          # every instance 1 cm along x
        biggest = int(np.argmax(inst[:, 3]))
        cases = [("one instance", [biggest]), ("all instances", list(range(n)))]      # (one instance: the device form still launches a thread per triangle of the scene)
        for what, ids in cases:
            r = frt.Renderer(fs, 64, 64, flags=frt.FLAG_PIPELINE)
            ids_host = np.asarray(ids, np.uint32)
            ids_dev = torch.tensor(ids, dtype=torch.int32, device=dev)
            mats_dev = torch.from_numpy(np.ascontiguousarray(moved[ids])).to(dev)
            host = timed(r, lambda: r.set_instance_transforms(ids_host, mats_dev.cpu().numpy()))      # (the copy waits for the caller's stream, as such a caller must)
            device = timed(r, lambda: r.set_instance_transforms(ids_dev, mats_dev))
            assert r.transform_rejects() == 0
            print(json.dumps({"scene": name, "tris": int(fs.counts()["tris"]), "instances": n, "moved": what, "moved_tris": int(inst[ids, 3].sum()),
                              "host_arrays_event_us": host[0], "host_arrays_wall_us": host[1], "device_tensors_event_us": device[0], "device_tensors_wall_us": device[1]}), flush=True)
            del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "colonnade"])
