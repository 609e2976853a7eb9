"""Cost of the ray queries (include/frt.h: frt_renderer_pick / _trace_closest / _trace_any) on the Cornell Box, the 82k-triangle
blob and the colonnade (tests/_scenes.py), 1920x1080:
  (a) the frame's 2,073,600 primary rays through frt_renderer_pick, beside the G-buffer stage of the same renderer in the same run (FRT_FLAG_TIMING,
      ms_stage[0] per launch): the same walk, without the stage's shading fetches and its four output streams;
  (b) as many rays with uniformly random origins in the scene's box and random directions, in random order (closest hit, any hit);
  (c) the host-pointer call for 1 ray and for 1,024 rays, wall clock: what a picking editor waits for.
(a) and (b) are the FRT_QUERY_DEVICE form between HIP events on the renderer's stream, median of 20. One JSON line per scene.
Usage: python tools/ray_query_time.py [cornell blob colonnade]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from frt._lib import check
from _oracle import Oracle
from instance_update_time import scene_of

REPS = 20


def event_ms(r, call):
    stream = torch.cuda.ExternalStream(r.stream_handle(0))
    call(); r.sync()      # warm: code object load, caches
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def wall_us(call):
    call()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    L = frt.lib()
    W, H = 1920, 1080
    n = W * H
    dev = torch.device("cuda", 0)
    for name in names:
        fs, _ = scene_of(name, orc)
        r = frt.Renderer(fs, W, H, flags=frt.FLAG_TIMING)
        cam = frt.CameraController().build_uniform(W / H, 0, fs.num_lights)
        # the G-buffer stage of this renderer: 24 frames, per launch
        for f in range(4):
            r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
        r.sync()
        s0 = r.stats()
        for f in range(4, 28):
            r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
        s1 = r.stats()
        g_ms = (s1["ms_stage"][0] - s0["ms_stage"][0]) / (s1["launches"][0] - s0["launches"][0])
        # (a) every pixel of the frame, row-major: the order in which a caller would list them (the G-buffer kernel walks 8x8 tiles per wave)
        ys, xs = np.mgrid[0:H, 0:W]
        xy = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)).to(dev)
        # ... and in the G-buffer kernel's own order (8x8 tiles, four to a 16x16 block), to separate the order from the kernel
        ty, tx = np.mgrid[0:(H + 15) // 16, 0:(W + 15) // 16]
        lane = np.arange(256); wave = lane >> 6; l = lane & 63
        px = (tx.ravel()[:, None] * 16 + (wave & 1) * 8 + (l & 7)).ravel(); py = (ty.ravel()[:, None] * 16 + (wave >> 1) * 8 + (l >> 3)).ravel()
        keep = (px < W) & (py < H)
        xy_tiled = torch.from_numpy(np.stack([px[keep], py[keep]], axis=1).astype(np.int32)).to(dev)
        hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        pick = lambda t: (lambda: check(L.frt_renderer_pick(r._h, C.byref(cam), n, t.data_ptr(), hits.data_ptr(), frt.QUERY_DEVICE)))
        pick_ms = event_ms(r, pick(xy))
        pick_tiled_ms = event_ms(r, pick(xy_tiled))
        hit_share = float((hits[:, 3] != -1).float().mean().item())
        # (b) random rays in the scene's box
        tris = fs.get("tris")
        v = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = v.min(axis=0), v.max(axis=0)
        rng = np.random.default_rng(1)
        o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = torch.from_numpy(frt.scene.ray_args(o, d, 0.001, 1000.0)).to(dev)
        torch.cuda.synchronize()
        rnd_ms = event_ms(r, lambda: check(L.frt_renderer_trace_closest(r._h, n, rays.data_ptr(), hits.data_ptr(), frt.QUERY_DEVICE)))
        rnd_hit = float((hits[:, 3] != -1).float().mean().item())
        any_ms = event_ms(r, lambda: check(L.frt_renderer_trace_any(r._h, n, rays.data_ptr(), occ.data_ptr(), frt.QUERY_DEVICE)))
        # (c) the host-pointer call
        h_rays = frt.scene.ray_args(o[:1024], d[:1024], 0.001, 1000.0); h_hits = np.zeros((1024, 8), np.uint32)
        one_us = wall_us(lambda: check(L.frt_renderer_trace_closest(r._h, 1, h_rays.ctypes.data, h_hits.ctypes.data, 0)))
        k_us = wall_us(lambda: check(L.frt_renderer_trace_closest(r._h, 1024, h_rays.ctypes.data, h_hits.ctypes.data, 0)))
        h_xy = np.array([[W // 2, H // 2]], np.uint32)
        pick_us = wall_us(lambda: check(L.frt_renderer_pick(r._h, C.byref(cam), 1, h_xy.ctypes.data, h_hits.ctypes.data, 0)))
        t = r.tree_stats()
        mr = lambda ms: round(n / ms / 1e3, 1)
        print(json.dumps({"scene": name, "tris": int(fs.counts()["tris"]), "quad_nodes": t["quad_nodes"], "stack_rows": t["quad_stack_need"] + 1, "rays": n,
                          "ms_gbuffer_stage": round(g_ms, 4), "mrays_gbuffer_stage": mr(g_ms),
                          "ms_pick_row_major": round(pick_ms, 4), "mrays_pick_row_major": mr(pick_ms),
                          "ms_pick_tile_order": round(pick_tiled_ms, 4), "mrays_pick_tile_order": mr(pick_tiled_ms), "primary_hit_share": round(hit_share, 3),
                          "ms_random_closest": round(rnd_ms, 4), "mrays_random_closest": mr(rnd_ms), "random_hit_share": round(rnd_hit, 3),
                          "ms_random_any": round(any_ms, 4), "mrays_random_any": mr(any_ms),
                          "us_host_call_1_ray": round(one_us, 1), "us_host_call_1024_rays": round(k_us, 1), "us_host_pick_1_pixel": round(pick_us, 1)}), flush=True)
        del r


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
