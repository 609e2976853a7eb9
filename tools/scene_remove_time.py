"""Cost of taking things out of a running renderer (include/frt.h: frt_renderer_remove_materials, _remove_meshes, _remove_texture, _remove_lights; DESIGN.md
section 16) on the Cornell Box and the 82k-triangle blob (tests/_scenes.py): microseconds per call (HIP events on the renderer's stream around the call,
median of 20; each measured removal follows an add that is not measured, so every call finds the replica in the same state) for one material, a
20,480-triangle icosphere mesh, one texture layer and one registered quad light; and, for comparison, what each replaces: the surviving builder calls on
a new host scene, build() and a new Renderer. One JSON line per scene.
Usage: python tools/scene_remove_time.py [cornell blob]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import frt
from _oracle import Oracle
from instance_update_time import scene_of
from instance_edit_time import event_us


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    ico = frt.geometry.create_sphere(5)                               # 20 * 4^5 = 20,480 triangles
    mat = frt.material_new([0.3, 0.5, 0.7, 1.0])
    y, x = np.mgrid[0:1024, 0:1024]
    layer = np.stack([(x * 7 + y * 3) % 256, (x ^ y) % 256, (x // 4) % 256, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    light_m = np.eye(4, dtype=np.float32).reshape(16) * np.float32(0.2); light_m[15] = 1.0; light_m[13] = 0.9
    white = (1.0, 1.0, 1.0)
    for name in names:
        fs, rebuild = scene_of(name, orc)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights)); r.sync()
        rec = {"scene": name, "tris": int(fs.counts()["tris"]), "icosphere_tris": int(len(ico.indices) // 3)}
        # (add, remove what it returned): the add puts the replica back, the removal is what is measured
        pairs = {"remove_materials": (lambda: r.add_materials(mat), lambda i: r.remove_materials(i)),
                 "remove_meshes": (lambda: r.add_meshes(ico), lambda i: r.remove_meshes(i)),
                 "remove_texture": (lambda: r.add_texture(0, layer), lambda i: r.remove_texture(0, i)),
                 "remove_lights": (lambda: r.register_quad_light(0, light_m, white, 5.0), lambda i: r.remove_lights(i))}
        for what, (add, remove) in pairs.items():
            remove(add())                                             # (the first call allocates the spare buffers and the staging block)
            us = []
            for _ in range(20):
                i = add(); r.sync()
                us.append(event_us(r, lambda: remove(i)))
            rec[f"us_{what}"] = round(float(np.median(us)), 1)
        for what in pairs:                                            # what a removal replaces: the scene without the thing, from scratch
            t0 = time.perf_counter()
            fs2 = rebuild()
            r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE); r2.sync()
            rec[f"s_host_{what}_build_and_recreate"] = round(time.perf_counter() - t0, 3)
            del r2
        print(json.dumps(rec), flush=True)
        del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob"])
