"""Cost of the material, light and texture edits (include/frt.h: frt_renderer_set_materials, _set_instance_materials, _set_light_emission, _set_texture;
DESIGN.md section 13) on the Cornell Box, the 82k-triangle blob and the 246k-triangle colonnade (tests/_scenes.py): microseconds per call (HIP events
on the renderer's stream around the call, median of 20) for one material, all materials, the material of the largest instance, one light and one
texture layer, and the host rebuild + renderer re-create they replace. One JSON line per scene.
Usage: python tools/scene_edit_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import scene_of


def call_us(r, call, reps=20):
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    for name in names:
        fs, rebuild = scene_of(name, orc)
        inst, mats, lights = fs.get("instances"), fs.get("materials"), fs.get("lights")
        biggest = int(np.argmax(inst[:, 3]))
        emission = lights[0, 12:16].view(np.float32)
        layer = np.full((1024, 1024, 4), 255, np.uint8)                  # colour layer 0 as the builder makes it: the scene stays as it is
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights)); r.sync()
        us = {"us_one_material": call_us(r, lambda: r.set_materials([0], [mats[0]])),
              "us_all_materials": call_us(r, lambda: r.set_materials(np.arange(len(mats)), list(mats))),
              "us_one_instance_material": call_us(r, lambda: r.set_instance_materials([biggest], [int(inst[biggest, 1])])),
              "us_one_light": call_us(r, lambda: r.set_light_emission(0, emission[0:3], float(emission[3]))),
              "us_one_texture_layer": call_us(r, lambda: r.set_texture("color", 0, layer))}
        t0 = time.perf_counter()
        fs2 = rebuild()
        r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE)
        r2.sync()
        rebuild_s = time.perf_counter() - t0
        rec = {"scene": name, "tris": int(fs.counts()["tris"]), "instances": len(inst), "materials": len(mats), "one_instance_tris": int(inst[biggest, 3])}
        rec.update({k: round(v, 1) for k, v in us.items()})
        rec["s_rebuild_and_recreate"] = round(rebuild_s, 3)
        print(json.dumps(rec), flush=True)
        del r, r2


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
