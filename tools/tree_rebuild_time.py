"""Cost and worth of rebuilding a renderer's tree on the device (include/frt.h: frt_renderer_rebuild_tree; DESIGN.md section 11, "Rebuild") on the Cornell
Box, the 82k-triangle blob and the 246k-triangle colonnade (tests/_scenes.py), 1920x1080, depth 8, two-stream schedule. Per scene, in a strongly moved
pose: the wall time of rebuild_tree() (first call, which allocates, and the median of 20 more), the device memory the first call takes, the host
rebuild + renderer re-create the call replaces, and the frame time over four trees measured alternately in one session: (i) a scene freshly
host-built in the moved pose, (ii) the original tree refit, (iii) refit + device rebuild, (iv) refit + refined device rebuild (quality="sah":
its call times, the device memory of its first call, its clustering iterations). node_term of all four trees by tests/_tree_cost.py. One JSON
line per scene.
Usage: python tools/tree_rebuild_time.py [cornell blob colonnade]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-raytracing-wgpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import frt
from _oracle import Oracle
from instance_update_time import frame_ms
from _tree_cost import tree_cost


def _ry(a):
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)      # column-major m[c, r]
    return m


def strong_moves(name, inst):
    """{instance id: column-major 4x4}. Cornell Box: the tall box across the room and the sphere light to the opposite corner. Elsewhere every instance
    of the largest mesh turns about its own origin and moves by up to a third of the scene's width (deterministic)."""
    cur = inst[:, 5:21].view(np.float32).reshape(-1, 4, 4)
    if name == "cornell":
        from test_tree_rebuild_gpu import big_moves
        return big_moves(frt)
    big = np.flatnonzero(inst[:, 3] == inst[:, 3].max())
    origins = cur[:, 3, :3]
    width = float(np.ptp(origins[:, [0, 2]], axis=0).max()) or 1.0
    rng = np.random.default_rng(7)
    out = {}
    for k in big:
        m = cur[k].copy()
        lin = _ry(rng.uniform(0.5, 2.5))
        m[:3, :3] = (m[:3, :3] @ lin[:3, :3]).astype(np.float32)                          # rows are columns here: M' = RY * M on the linear part
        m[3, 0] += np.float32(rng.uniform(-1, 1) * width / 3 if len(big) > 1 else 0.25)
        m[3, 2] += np.float32(rng.uniform(-1, 1) * width / 3 if len(big) > 1 else 0.15)
        if len(big) == 1:
            m[3, 1] += np.float32(0.2)
        out[int(k)] = m.reshape(16)
    return out


def builders(name, orc):
    """(build(), build_moved(moves)): the scene as tests/_scenes.py issues it, and the same calls with instance k at moves[k]."""
    import _scenes
    if name == "cornell":
        from test_instance_update import cornell
        return frt.scenes.create_cornell_box, lambda moves: cornell(frt, moves)
    make = (lambda: _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)[0]) if name == "blob" else (lambda: _scenes.colonnade(frt, orc)[0])

    def moved(moves):
        plain, count = _scenes.DualBuilder.add_instance, [0]

        def add_instance(self, mesh, mat, m):
            k = count[0]; count[0] += 1
            return plain(self, mesh, mat, moves[k] if k in moves else m)
        _scenes.DualBuilder.add_instance = add_instance
        try:
            return make()
        finally:
            _scenes.DualBuilder.add_instance = plain
    return make, moved


def main(names):
    orc = Oracle(os.path.join(ROOT, "oracle", "_build", "liborc.so"))
    W, H = 1920, 1080
    for name in names:
        build, build_moved = builders(name, orc)
        fs = build()
        moves = strong_moves(name, fs.get("instances"))
        ids = sorted(moves)
        mats = np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])
        t0 = time.perf_counter()
        fresh = build_moved(moves)
        r_fresh = frt.Renderer(fresh, W, H, flags=frt.FLAG_PIPELINE)
        r_fresh.sync()
        host_s = time.perf_counter() - t0                                                 # what a user without the call pays: host build + re-create
        r_refit, r_rebuilt, r_sah = (frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE) for _ in range(3))
        ms_rest = frame_ms(r_refit, W, H, fs.num_lights)
        for r in (r_refit, r_rebuilt, r_sah):
            r.set_instance_transforms(ids, mats)
        r_rebuilt.sync(); r_sah.sync(); torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter(); r_rebuilt.rebuild_tree(); first_ms = (time.perf_counter() - t0) * 1e3
        free1 = torch.cuda.mem_get_info()[0]
        calls = []
        for _ in range(20):
            t0 = time.perf_counter(); r_rebuilt.rebuild_tree(); calls.append((time.perf_counter() - t0) * 1e3)
        free2 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter(); r_sah.rebuild_tree("sah"); sah_first_ms = (time.perf_counter() - t0) * 1e3
        free3 = torch.cuda.mem_get_info()[0]
        sah_calls = []
        for _ in range(20):
            t0 = time.perf_counter(); r_sah.rebuild_tree("sah"); sah_calls.append((time.perf_counter() - t0) * 1e3)
        sah_ms = float(np.median(sah_calls))
        assert r_rebuilt.read_scene("tri_slots").shape == fresh.get("tri_slots").shape
        trees = {"fresh": r_fresh, "refit": r_refit, "rebuilt": r_rebuilt, "sah": r_sah}
        node_term = {k: round(tree_cost(r.read_scene("quad_nodes"))["node_term"], 4) for k, r in trees.items()}
        ms = {k: [] for k in trees}
        for _ in range(5):                                                                # alternately, one session
            for k, r in trees.items():
                ms[k].append(frame_ms(r, W, H, fs.num_lights))
        call_ms = float(np.median(calls))
        print(json.dumps({"scene": name, "tris": int(fs.counts()["tris"]), "moved_instances": len(ids),
                          "ms_rebuild_first_call": round(first_ms, 3), "ms_rebuild_call": round(call_ms, 3), "ms_rebuild_call_min_max": [round(min(calls), 3), round(max(calls), 3)],
                          "bytes_first_call": int(free0 - free1), "bytes_later_calls": int(free1 - free2),
                          "s_host_rebuild_and_recreate": round(host_s, 3), "host_over_call": round(host_s * 1e3 / call_ms, 1),
                          "ms_frame_rest_pose": round(ms_rest, 3),
                          "ms_frame": {k: round(float(np.median(v)), 3) for k, v in ms.items()}, "ms_frame_runs": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                          "tree_fresh": {k: fresh.tree_stats()[k] for k in ("quad_nodes", "quad_stack_need")}, "tree_refit": r_refit.tree_stats(),
                          "tree_rebuilt": r_rebuilt.tree_stats(), "tree_sah": r_sah.tree_stats(),
                          "ms_sah_first_call": round(sah_first_ms, 3), "ms_sah_call": round(sah_ms, 3), "ms_sah_call_min_max": [round(min(sah_calls), 3), round(max(sah_calls), 3)],
                          "sah_over_morton_call": round(sah_ms / call_ms, 2), "bytes_sah_first_call": int(free2 - free3),
                          "sah_refined_scratch_kib": r_sah.rebuild_stats()["refined_scratch_kib"], "sah_iterations": r_sah.rebuild_stats()["iterations"],
                          "sah_fell_back": r_sah.rebuild_stats()["fell_back"], "node_term": node_term}), flush=True)
        del trees, r_fresh, r_refit, r_rebuilt, r_sah


if __name__ == "__main__":
    main(sys.argv[1:] or ["cornell", "blob", "colonnade"])
