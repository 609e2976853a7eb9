"""Cost of importing into a running renderer (include/frt.h: frt_renderer_add_meshes, _add_materials, _add_texture, _register_quad_light; DESIGN.md
section 15) on the Cornell Box and the 82k-triangle blob (tests/_scenes.py): microseconds per call (HIP events on the renderer's stream around the call,
median of 20; nothing can be removed again, so every call finds the replica one step larger and some calls grow a capacity) for a 20,480-triangle
icosphere, 16 materials, one texture layer and one registered quad light; and, for comparison, what each replaces: the same builder calls on the host
scene, build() and a new Renderer. One JSON line per scene.
Usage: python tools/scene_grow_time.py [cornell blob]"""
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
    mats = [frt.material_new([0.1 + 0.05 * k, 0.5, 0.9 - 0.05 * k, 1.0]) for k in range(16)]
    y, x = np.mgrid[0:1024, 0:1024]
    layer = np.stack([(x * 7 + y * 3) % 256, (x ^ y) % 256, (x // 4) % 256, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    light_m = np.eye(4, dtype=np.float32).reshape(16) * np.float32(0.2); light_m[15] = 1.0; light_m[13] = 0.9
    white = (1.0, 1.0, 1.0)
    for name in names:
        fs, rebuild = scene_of(name, orc)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
        r.render(frt.CameraController().build_uniform(W / H, 0, fs.num_lights)); r.sync()
        rec = {"scene": name, "tris": int(fs.counts()["tris"]), "icosphere_tris": int(len(ico.indices) // 3)}
        calls = {"add_meshes": lambda: r.add_meshes(ico), "add_materials": lambda: r.add_materials(mats), "add_texture": lambda: r.add_texture(0, layer),
                 "register_quad_light": lambda: r.register_quad_light(0, light_m, white, 5.0)}
        for what, call in calls.items():
            call()                                                        # (the first call allocates the staging blocks and gives the pools their capacities)
            rec[f"us_{what}"] = round(float(np.median([event_us(r, call) for _ in range(20)])), 1)
        rec["growths"] = r.pool_counts()["growths"]
        host = {"add_meshes": lambda s: s.add_mesh(ico), "add_materials": lambda s: [s.add_material(m) for m in mats], "add_texture": lambda s: s.add_color_texture(layer),
                "register_quad_light": lambda s: s.register_quad_light(0, light_m, white, 5.0)}
        for what, call in host.items():
            fs2 = rebuild()
            t0 = time.perf_counter()
            call(fs2); fs2.build()
            r2 = frt.Renderer(fs2, W, H, flags=frt.FLAG_PIPELINE); r2.sync()
            rec[f"s_host_{what}_build_and_recreate"] = round(time.perf_counter() - t0, 3)
            del r2
        print(json.dumps(rec), flush=True)
        del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob"])
