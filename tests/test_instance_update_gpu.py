"""Moving instances on the device (include/frt.h: frt_renderer_set_instance_transforms): the refit replica equals the host
reference bit for bit, and renderers after a move render exactly what a renderer over a freshly built scene renders (closest hits break ties by
flattened triangle id, so the image depends on the triangles only, not on the tree's shape)."""
import os
import numpy as np
import pytest
from test_hostcheck_parity import compare_all
from test_instance_update import cornell, cornell_moves, cornell_meshes, move, oracle_scene, TALL_BOX, SPHERE_LIGHT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICA = ("tri_slots", "pair_nodes", "quad_nodes", "instances_dev", "lights")


@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


def _moves_for(frt, which, fs):
    from frt.scenes import _T, _S, _RY, _mul
    inst = fs.get("instances")
    if which == "cornell":
        return cornell_moves(frt)
    if which == "restir":      # the metal cube (last instance) and three of the light spheres (their lights were added with add_light: they stay)
        n = len(inst)
        return {n - 1: _mul(_T(0.3, -0.4, 0.2), _RY(0.7), _S(0.6)), 2: _mul(_T(-4.0, -0.5, -4.0), _S(0.08)), 50: _mul(_T(0.5, -0.8, 0.5), _S(0.05)),
                51: _mul(_T(0.6, -0.8, 0.5), _S(0.05))}
    return {6: _mul(_T(0.1, -0.35, 0.05), _RY(0.5), _S(0.55))}      # the 82k-triangle blob


@pytest.mark.parametrize("which", ["cornell", "restir", "blob82k"])
def test_device_replica_matches_the_host_reference(gpu, orc, which):
    frt = gpu
    import _scenes
    if which == "cornell":
        fs = frt.scenes.create_cornell_box()
    elif which == "restir":
        fs = frt.scenes.create_restir_scene()
    else:
        fs, _ = _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)
    r = frt.Renderer(fs, 32, 24, flags=frt.FLAG_PIPELINE)
    before = {w: r.read_scene(w) for w in REPLICA}
    for w in REPLICA:
        assert before[w].tobytes() == fs.get(w).tobytes(), f"{which} {w} at create"
    cam = frt.CameraController().build_uniform(32 / 24, 0, fs.num_lights)
    r.render(cam)
    moves = _moves_for(frt, which, fs)
    ids = sorted(moves)
    mats = np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])
    r.set_instance_transforms(ids, mats)
    fs.set_instance_transforms(ids, mats)
    for w in REPLICA:
        got, want = r.read_scene(w), fs.get(w)
        assert got.tobytes() == want.tobytes(), f"{which} {w}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
    assert r.read_scene("tri_slots").tobytes() != before["tri_slots"].tobytes()


def _render_all(frt, r, W, H, nl, frames, first=0):
    cams = [frt.CameraController().build_uniform(W / H, f, nl) for f in range(first, first + frames)]
    for cam in cams:
        r.render(cam)
    return cams


@pytest.mark.parametrize("flags", [0, 8], ids=["one stream", "pipeline"])
def test_moved_renderer_matches_a_fresh_build_and_the_oracle(gpu, orc, flags):
    frt = gpu
    W, H, depth, frames = 128, 128, 8, 3
    moves = cornell_moves(frt)
    fresh = cornell(frt, moves)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=depth, flags=flags)
    _render_all(frt, r, W, H, fresh.num_lights, 2)
    r.set_instance_transforms(sorted(moves), np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in sorted(moves)]))
    r.clear()
    rf = frt.Renderer(fresh, W, H, max_depth=depth, flags=flags)
    ro = oracle_scene(orc, fresh, cornell_meshes(frt)).renderer(W, H, depth, False, 16)      # brute force: nothing of either tree
    for f in range(frames):
        cam = frt.CameraController().build_uniform(W / H, f, fresh.num_lights)
        r.render(cam); rf.render(cam); ro.render(cam)
        compare_all(r.read_buffer, rf.read_buffer, f, "moved vs fresh build")
        compare_all(r.read_buffer, ro.read, f, "moved vs brute-force oracle")
    st, sf, so = r.stats(), rf.stats(), ro.stats()["total"]
    assert (st["rays_closest"], st["rays_any"]) == (sf["rays_closest"], sf["rays_any"]) == (so["closest"], so["any"])


@pytest.mark.parametrize("flags", [8, 8 | 16], ids=["pipeline", "pipeline + third set"])
def test_mid_sequence_move_with_the_pipeline(gpu, flags):
    """Render 3 frames, move, render 3 more: the two-stream schedule (whose next frame's G-buffer + T-trace ran ahead under the old geometry)
    equals the one-stream schedule on every buffer of every frame. With two G-buffer sets the frame running ahead writes the set of the
    previous logical slot (frt_renderer.hip: alloc_g), which a read through the ABI then shows: before a move it holds the same pixels, after
    it the new geometry's, so there only the frame's own slot of the G-buffer targets is compared."""
    frt = gpu
    W, H = 96, 64
    fs = frt.scenes.create_cornell_box()
    moves = cornell_moves(frt)
    ids = sorted(moves)
    mats = np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])
    a, b = frt.Renderer(fs, W, H), frt.Renderer(fs, W, H, flags=flags)
    third = bool(flags & 16)
    for f in range(6):
        if f == 3:
            a.set_instance_transforms(ids, mats); b.set_instance_transforms(ids, mats)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        a.render(cam); b.render(cam)
        for buf in range(8):
            for idx in ((0, 1) if buf in (0, 1, 2, 4, 7) else (0,)):
                if buf in (0, 1, 2) and idx != f % 2 and not third:
                    continue
                g, w = b.read_buffer(buf, idx), a.read_buffer(buf, idx)
                assert g.tobytes() == w.tobytes(), f"frame {f} buffer {buf}[{idx}]"
    sa, sb = a.stats(), b.stats()
    assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    assert sb["discarded_speculations"] >= 1          # the frame speculated under the old geometry was dropped


def test_multi_renderer_strips_match_one_renderer(gpu):
    frt = gpu
    W, H = 128, 96
    fs = frt.scenes.create_cornell_box()
    moves = cornell_moves(frt)
    ids = sorted(moves)
    mats = np.stack([np.asarray(moves[k], np.float32).reshape(16) for k in ids])
    multi = frt.MultiRenderer(fs, W, H, [0, 0])
    one = frt.Renderer(fs, W, H, flags=frt.FLAG_PIPELINE)
    for f in range(4):
        if f == 2:
            multi.set_instance_transforms(ids, mats); one.set_instance_transforms(ids, mats)
        cam = frt.CameraController().build_uniform(W / H, f, fs.num_lights)
        multi.render(cam); one.render(cam)
    multi.sync()
    assert multi.read_accum().tobytes() == one.read_accum().tobytes()
    assert multi.read_display().tobytes() == one.read_display().tobytes()
    with pytest.raises(frt.FrtError):
        multi.set_instance_transforms([99], mats[:1])


def test_renderer_argument_and_state_errors(gpu):
    frt = gpu
    fs = frt.scenes.create_cornell_box()
    r = frt.Renderer(fs, 32, 32)
    eye = np.eye(4, dtype=np.float32)
    sing = eye.copy(); sing[1, 1] = 0.0
    nan = eye.copy(); nan[3, 0] = np.nan
    for ids, m in (([9], [eye]), ([0], [sing]), ([0], [nan])):
        with pytest.raises(frt.FrtError):
            r.set_instance_transforms(ids, m)
    cam = frt.CameraController().build_uniform(1.0, 0, fs.num_lights)
    r.render_phases(cam, frt.PHASE_GBUFFER)
    with pytest.raises(frt.FrtError):
        r.set_instance_transforms([TALL_BOX], [eye])          # a frame is open
    r.render_phases(cam, frt.PHASE_ALL); r.end_frame()
    r.set_instance_transforms([TALL_BOX, SPHERE_LIGHT], [eye, eye])
    assert r.read_scene("tri_slots").tobytes() == move(fs, {TALL_BOX: eye, SPHERE_LIGHT: eye}).get("tri_slots").tobytes()


def test_experiments_build_refuses_the_wide_walk(gpu):
    import subprocess, sys
    exp = os.path.join(ROOT, "fast-raytracing-wgpu_amd", "lib", "libfrt_exp.so")
    code = ("import sys, numpy as np; sys.path[:0] = [%r]; import frt\n"
            "fs = frt.scenes.create_cornell_box()\n"
            "r = frt.Renderer(fs, 32, 32, flags=frt.FLAG_WALK_WIDE)\n"
            "try:\n    r.set_instance_transforms([8], [np.eye(4, dtype=np.float32)])\n    print('ACCEPTED')\n"
            "except frt.FrtError as e:\n    print('REFUSED', e)\n"
            "q = frt.Renderer(fs, 32, 32)\nq.set_instance_transforms([8], [np.eye(4, dtype=np.float32)])\nprint('QUAD OK')\n") % os.path.join(ROOT, "fast-raytracing-wgpu_amd")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FRT_LIB=exp))
    assert p.returncode == 0, p.stderr[-3000:]
    assert "REFUSED" in p.stdout and "QUAD OK" in p.stdout, p.stdout
