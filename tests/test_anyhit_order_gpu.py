"""The frame kernels with the any-hit node step that enters the nearest hit child and stacks the others in slot order (csrc/frt_trace.hpp:
trace4<ANY = true>): every buffer of every frame and both ray counts against the brute-force oracle, on the Cornell Box, a one-leaf scene and a tree
at the stack limit of 31; 64x48 at depth 8 for two frames (the second one merges and reuses real history) and one 40x24 frame (partial tiles);
with the while-while kernels and with the voting kernels (FRT_WALK_VOTE, csrc/frt_renderer_state.hpp: walk_votes, read when a renderer is made)."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import oracle_scene
from test_instance_update_gpu import gpu      # noqa: F401  (gpu: the module's device fixture)
from test_lds_top_gpu import scene_list

pytestmark = pytest.mark.gpu
_ORACLE = {}      # (scene, W, H, frames) -> (per frame: {(buffer, index): bytes}, (closest, any)): computed once, shared by both walks, never changed


def oracle_frames(frt, orc, which, lst, fs, W, H, frames):
    key = (which, W, H, frames)
    if key not in _ORACLE:
        ro = oracle_scene(orc, fs, lst.meshes).renderer(W, H, 8, False, 16)
        per_frame = []
        for f in range(frames):
            ro.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
            per_frame.append({(b, idx): ro.read(b, idx).copy() for b in range(8) for idx in ((0, 1) if b in (0, 1, 2, 4, 7) else (0,))})
        so = ro.stats()["total"]
        _ORACLE[key] = (per_frame, (so["closest"], so["any"]))
    return _ORACLE[key]


@pytest.mark.parametrize("vote", [0, 1], ids=["while-while", "voting"])
@pytest.mark.parametrize("W,H,frames", [(64, 48, 2), (40, 24, 1)])
@pytest.mark.parametrize("which", ["cornell", "one leaf", "stack need 31"])
def test_frames_equal_the_oracle_with_either_walk(gpu, orc, monkeypatch, which, W, H, frames, vote):
    frt = gpu
    lst = scene_list(frt, which)
    fs = lst.build(frt)
    per_frame, rays = oracle_frames(frt, orc, which, lst, fs, W, H, frames)
    monkeypatch.setenv("FRT_WALK_VOTE", str(vote))
    r = frt.Renderer(fs, W, H, max_depth=8)
    for f in range(frames):
        r.render(frt.CameraController().build_uniform(W / H, f, fs.num_lights))
        compare_all(r.read_buffer, lambda b, idx: per_frame[f][b, idx], f, f"{which} {W}x{H} {'voting' if vote else 'while-while'}: vs brute-force oracle")
    st = r.stats()
    assert (st["rays_closest"], st["rays_any"]) == rays
    assert st["rays_any"] > 0 or fs.num_lights == 0      # (the one-leaf scene has no light: nothing fires an any-hit ray there)
