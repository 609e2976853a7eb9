"""Regional continuation queues on a real MI355X (csrc/frt_mono.hpp: ContQueue::nsub; csrc/frt_kernels.hip: wave_reserve on a region's counter,
continue_kernel over (region, offset), per-region ray counters): every buffer of every frame and the exact ray counts against the oracle over
three frames, at queue geometries chosen to reach every path of the protocol. The geometry comes from FRT_QUEUE_REGIONS=<regions>[,<slots>],
which a renderer reads once when it is created (csrc/frt_renderer.hip)."""
import numpy as np
import pytest
from test_hostcheck_parity import compare_all

pytestmark = pytest.mark.gpu
FRAMES, DEPTH = 3, 8
SMALLEST, CHOSEN = 1, 16      # regions: one counter per queue, and the renderer's default (profiles/r12_experiments/regional_queues.md)
_oracle_frames = {}


@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


def cameras(frt, W, H):
    return [frt.CameraController().build_uniform(W / H, f, 2) for f in range(FRAMES)]


def oracle(frt, orc, W, H):
    """The oracle's buffers after each of the three frames and its ray totals: computed once per frame size, never changed."""
    if (W, H) not in _oracle_frames:
        fs = frt.scenes.create_cornell_box()
        os_ = orc.cornell(); os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
        ro = os_.renderer(W, H, DEPTH, True, 16)
        frames = []
        for cam in cameras(frt, W, H):
            ro.render(cam)
            frames.append({(b, idx): ro.read(b, idx).copy() for b in range(8) for idx in (0, 1)})
        so = ro.stats()["total"]
        _oracle_frames[W, H] = (frames, (so["closest"], so["any"]))
    return _oracle_frames[W, H]


def render_and_compare(frt, orc, W, H, ctx, after_frame=None, **opts):
    frames, rays = oracle(frt, orc, W, H)
    r = frt.Renderer(frt.scenes.create_cornell_box(), W, H, max_depth=DEPTH, **opts)
    for f, cam in enumerate(cameras(frt, W, H)):
        r.render(cam)
        compare_all(r.read_buffer, lambda b, idx: frames[f][b, idx], f, ctx)
        if after_frame:
            after_frame(f, r)
    st = r.stats()
    assert (st["rays_closest"], st["rays_any"]) == rays, ctx      # the regions' ray counters sum to the oracle's counts
    return st


@pytest.mark.parametrize("flags", [0, 8], ids=["plain", "side-stream"])
@pytest.mark.parametrize("cuts", [None, [2, 4]], ids=["one cut", "two cuts"])
@pytest.mark.parametrize("nsub", [SMALLEST, CHOSEN])
def test_ragged_frame(gpu, orc, monkeypatch, nsub, cuts, flags):
    """72x40: ragged in both directions, 15 workgroups. Two cuts: continue_kernel parks again, into its own region of the odd queue."""
    monkeypatch.setenv("FRT_QUEUE_REGIONS", str(nsub))
    st = render_and_compare(gpu, orc, 72, 40, f"72x40, {nsub} regions, cuts {cuts}, flags {flags}", cuts=cuts, flags=flags)
    assert st["queue_overflow"] == 0, st      # the default capacity of a small frame holds every pixel, region by region


@pytest.mark.parametrize("flags", [0, 8], ids=["plain", "side-stream"])
def test_forced_overflow_of_some_regions_grows_the_queue(gpu, orc, monkeypatch, flags):
    """16 regions of 64 slots for 15 workgroups of 256 paths: a workgroup has a region to itself and parks up to 128 paths at the second bounce
    — more than 64 where the tile sees the boxes and the floor —, region 15 has no workgroup. The surplus paths finish in place (same pixels,
    same counts), the overflow is counted and reaches the host, and the queue is grown."""
    monkeypatch.setenv("FRT_QUEUE_REGIONS", "16,1024")
    seen = {}

    def after_frame(f, r):
        if f == 0:
            seen["first"] = r.stats()      # (stats also looks at the overflow counters and grows the queues)
    st = render_and_compare(gpu, orc, 72, 40, f"72x40, 16 regions of 64 slots, flags {flags}", after_frame=after_frame, cuts=[2, 4], flags=flags)
    assert seen["first"]["queue_overflow"] > 0, seen
    assert seen["first"]["queue_capacity"] > 1024 and st["queue_capacity"] >= seen["first"]["queue_capacity"], (seen, st)


def test_fewer_workgroups_than_regions(gpu, orc, monkeypatch):
    """16x16: one workgroup, all regions but one stay empty — every continuation workgroup but one leaves at once."""
    monkeypatch.setenv("FRT_QUEUE_REGIONS", str(CHOSEN))
    render_and_compare(gpu, orc, 16, 16, "16x16, one workgroup", cuts=[2, 4])


def test_regions_smaller_than_a_wave(gpu, orc, monkeypatch):
    """A capacity of 512 given by the caller (never grown) in 16 regions: 32 slots per region, less than one wave parks at a time. Every
    workgroup's region overflows: one report per region, the surplus counted."""
    monkeypatch.setenv("FRT_QUEUE_REGIONS", str(CHOSEN))
    st = render_and_compare(gpu, orc, 72, 40, f"72x40, {CHOSEN} regions of {512 // CHOSEN} slots", cuts=[2, 4], queue_capacity=512)
    assert 512 // CHOSEN < 64 and st["queue_overflow"] > 0 and st["queue_capacity"] == 512, st


@pytest.mark.parametrize("flags", [0, 8], ids=["plain", "side-stream"])
def test_strips_share_the_regions_between_interior_and_edge_launches(gpu, orc, monkeypatch, flags):
    """72x48 in two strips of 24 rows: the strip boundary cuts a tile row, and the spatial stage of a strip is an interior launch and an edge
    launch that park into the same regions, each by its own block index. Rows and summed ray counts against the whole frame (the oracle's)."""
    from frt.dist import StripPlan
    from test_gpu_parity import _strip_frame
    frt = gpu
    monkeypatch.setenv("FRT_QUEUE_REGIONS", str(CHOSEN))
    W, H = 72, 48
    frames, rays = oracle(frt, orc, W, H)
    fs = frt.scenes.create_cornell_box()
    plans = [StripPlan(H, 2, k) for k in range(2)]
    strips = [frt.Renderer(fs, W, H, max_depth=DEPTH, rows=(p.row_begin, p.row_end), cuts=[2, 4], flags=flags) for p in plans]
    for f, cam in enumerate(cameras(frt, W, H)):
        _strip_frame(frt, strips, plans, cam, f)
        for s, p in zip(strips, plans):
            for b, idx in ((7, f % 2), (6, 0)):      # what a strip owns of the frame: its rows of the accumulation and of the display
                assert s.read_buffer(b, idx)[p.row_begin:p.row_end].tobytes() == frames[f][b, idx][p.row_begin:p.row_end].tobytes(), (f, p.rank, b)
    sts = [s.stats() for s in strips]
    assert (sum(st["rays_closest"] for st in sts), sum(st["rays_any"] for st in sts)) == rays      # halo rows are not counted twice
