"""The traced kernels under both LDS budgets of the launch plan (csrc/frt_kernels.hpp: traced_lds_budget; tests/test_lds_budget.py holds the plan
itself): 32 KiB per workgroup, the default, and the 40 KiB that FRT_LDS_BUDGET=40 asks for when a renderer is created. A budget changes how many of
the tree's first nodes a workgroup copies behind its stack rows (the Cornell Box: 63 or 127 of 326) and nothing a pixel can see: every buffer and the
ray counts of the two must be the same bytes, and the oracle's. The smallest shapes at which a wrong row count, a node index past the copy or a
clobbered register shows: the Cornell Box at 64x48, depth 8, two frames, on one stream and pipelined; one 32x32 frame of a tree whose stack need is
the limit of 31, where seven nodes fit; one 32x24 frame of the two-sphere scene, whose tree the voting kernels walk."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import oracle_scene
from test_instance_update_gpu import gpu      # noqa: F401  (the module's device fixture)
from test_lds_top_gpu import scene_list
from test_ray_query_gpu import two_spheres, VOTE_MIN_QUAD_NODES

pytestmark = pytest.mark.gpu
BUDGETS = (None, "40")      # FRT_LDS_BUDGET in KiB; None: the default, 32


def renderers(frt, monkeypatch, fs, w, h, flags=0):
    """One renderer per budget; the variable is read once, when a renderer is created."""
    out = []
    for kib in BUDGETS:
        if kib is None:
            monkeypatch.delenv("FRT_LDS_BUDGET", raising=False)
        else:
            monkeypatch.setenv("FRT_LDS_BUDGET", kib)
        out.append(frt.Renderer(fs, w, h, max_depth=8, flags=flags))
    monkeypatch.delenv("FRT_LDS_BUDGET", raising=False)
    return out


def frames_equal(frt, rs, ro, w, h, lights, frames, what):
    for f in range(frames):
        cam = frt.CameraController().build_uniform(w / h, f, lights)
        ro.render(cam)
        for r in rs:
            r.render(cam)
        for kib, r in zip(BUDGETS, rs):
            compare_all(r.read_buffer, ro.read, f, f"{what}, budget {kib or 32} KiB vs oracle")
        compare_all(rs[0].read_buffer, rs[1].read_buffer, f, f"{what}, 32 KiB vs 40 KiB")
    so = ro.stats()["total"]
    for kib, r in zip(BUDGETS, rs):
        st = r.stats()
        assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"]), f"{what}, budget {kib or 32} KiB"
        assert st["queue_overflow"] == 0


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_cornell_frames_under_both_budgets(gpu, orc, monkeypatch, flags):
    frt = gpu
    assert flags in (0, frt.FLAG_PIPELINE)
    W, H = 64, 48
    fs = frt.scenes.create_cornell_box()
    assert fs.tree_stats()["quad_nodes"] == 326 and fs.tree_stats()["quad_stack_need"] == 24
    os_ = orc.cornell()
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    frames_equal(frt, renderers(frt, monkeypatch, fs, W, H, flags), os_.renderer(W, H, 8, True, 16), W, H, fs.num_lights, 2, "cornell 64x48")


def test_frame_of_a_tree_at_the_stack_limit(gpu, orc, monkeypatch):
    frt = gpu
    W = H = 32
    lst = scene_list(frt, "stack need 31")
    fs = lst.build(frt)
    assert fs.tree_stats()["quad_stack_need"] == 31 and 7 < fs.tree_stats()["quad_nodes"] <= 71      # more nodes than 32 KiB leave room for behind 31 rows (7); 40 KiB hold the whole tree
    ro = oracle_scene(orc, fs, lst.meshes).renderer(W, H, 8, False, 16)
    frames_equal(frt, renderers(frt, monkeypatch, fs, W, H), ro, W, H, fs.num_lights, 1, "stack need 31, 32x32")


def test_frame_of_the_voting_kernels(gpu, orc, monkeypatch):
    frt = gpu
    W, H = 32, 24
    fs, os_ = two_spheres(frt, orc)
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    rs = renderers(frt, monkeypatch, fs, W, H)
    assert rs[0].tree_stats()["quad_nodes"] >= VOTE_MIN_QUAD_NODES
    frames_equal(frt, rs, os_.renderer(W, H, 8, True, 16), W, H, fs.num_lights, 1, "two spheres 32x24")
