"""The frame kernels' LDS is sized per launch from the scene's tree: one row per stack entry the tree needs, the shared words, and behind them a copy
of as many of the tree's first nodes as a 40 KiB workgroup leaves room for (csrc/frt_kernels.hpp: walk_lds_plan). 64x64 frames, depth 8, every
buffer of three frames and the ray counts against the oracle, on trees that meet each edge of that plan: the Cornell Box (more nodes than the copy
holds), trees smaller than the copy down to a single node, a tree whose stack need is the limit of 31 (the stack rows fill the allocation), and a
renderer whose tree — and with it the row count and the copy — changes between frames."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import oracle_scene
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from _instance_lists import SceneList, cornell_list, two_instance_list, trs

pytestmark = pytest.mark.gpu
W = H = 64
FRAMES = 3
SPHERE, TALL_BOX, TRI = 7, 8, 4      # instances / mesh of cornell_list


def chain(frt, lst, n):
    """n one-triangle instances shrinking by halves towards the room's centre: the builder peels one off per level, a thin deep tree."""
    ms = [trs(frt, (0.7 * 0.5 ** k, 0.3 * 0.5 ** k, 0.5 * 0.5 ** k), 0.25 * 0.5 ** k, 0.0) for k in range(n)]
    return lst.added([TRI] * n, [0] * n, ms), ms


def scene_list(frt, which):
    if which == "cornell":
        return cornell_list(frt)
    if which == "walls":
        return cornell_list(frt).removed([SPHERE, TALL_BOX])
    if which == "one leaf":
        base = two_instance_list(frt)
        return SceneList(base.meshes, base.materials, base.entries[:1])
    if which == "stack need 31":
        return chain(frt, cornell_list(frt).removed([SPHERE, TALL_BOX]), 54)[0]
    raise KeyError(which)


def frames_equal_oracle(frt, orc, lst, fs, renderers, what):
    """Every renderer of `renderers` against the brute-force oracle over the scene (nothing of any tree), frame by frame, and the ray counts."""
    ro = oracle_scene(orc, fs, lst.meshes).renderer(W, H, 8, False, 16)
    for f in range(FRAMES):
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        ro.render(cam)
        for r in renderers:
            r.render(cam)
            compare_all(r.read_buffer, ro.read, f, f"{what}: frame {f} vs brute-force oracle")
    so = ro.stats()["total"]
    for r in renderers:
        st = r.stats()
        assert (st["rays_closest"], st["rays_any"]) == (so["closest"], so["any"]), what


@pytest.mark.parametrize("which,nodes,need", [("cornell", 326, 24), ("walls", None, None), ("one leaf", 1, None), ("stack need 31", None, 31)])
def test_frames_equal_the_oracle(gpu, orc, which, nodes, need):
    frt = gpu
    lst = scene_list(frt, which)
    fs = lst.build(frt)
    ts = fs.tree_stats()
    print(f"{which}: {ts}")
    if nodes is not None:
        assert ts["quad_nodes"] == nodes
    if need is not None:
        assert ts["quad_stack_need"] == need
    if which == "walls":
        assert 1 < ts["quad_nodes"] < 71      # fewer than the copy holds at ANY stack need (71 nodes fit behind 31 stack rows)
    r = frt.Renderer(fs, W, H, max_depth=8)
    assert r.tree_stats()["quad_stack_need"] == ts["quad_stack_need"]
    frames_equal_oracle(frt, orc, lst, fs, [r], which)


def test_rows_and_copy_follow_the_tree(gpu, orc):
    """Instances added to a running renderer change the tree's stack need; the frames after the edit equal a fresh renderer's and the oracle's."""
    frt = gpu
    lst = cornell_list(frt)
    r = frt.Renderer(lst.build(frt), W, H, max_depth=8)
    for f in range(2):
        r.render(frt.CameraController().build_uniform(W / H, f, 2))
    before = r.tree_stats()
    after, ms = chain(frt, lst, 40)
    r.add_instances([TRI] * 40, [0] * 40, np.stack(ms), quality="sah")
    now = r.tree_stats()
    print(f"stack need {before['quad_stack_need']} -> {now['quad_stack_need']}, quad nodes {before['quad_nodes']} -> {now['quad_nodes']}")
    assert now["quad_stack_need"] != before["quad_stack_need"] and now["quad_stack_need"] <= 31
    fresh = after.build(frt)
    r.clear()
    frames_equal_oracle(frt, orc, after, fresh, [r, frt.Renderer(fresh, W, H, max_depth=8)], "after add_instances")
