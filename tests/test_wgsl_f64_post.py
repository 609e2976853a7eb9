"""The post / accumulate pass (post.wgsl main) against its float64 restatement (tests/_wgsl_f64.py: post_f64) on crafted inputs.
A real frame runs GBUFFER | TEMPORAL | SPATIAL; then the buffers post reads are overwritten through write_rows with data that reaches
every branch (prev_uv exactly 0 / 1, outside, NaN; speed around 0.5 and 2; history taps off the image; bilateral weights summing to
<= 0.001; radiance up to the f16 maximum; history near the tonemap singularity; jitter within and beyond a pixel), POST runs alone,
and accum / display are compared pixel by pixel. Runs on the oracle (CPU suite) and on libfrt.so (-m gpu, where the kernel must also
equal the oracle bit for bit on the same crafted inputs)."""
import numpy as np
import pytest
import _wgsl_f64 as R

GPOS, GNORMAL, GALBEDO, GMOTION, RAW, DISPLAY, ACCUM = 0, 1, 2, 3, 5, 6, 7
SIZES = [(1, 1), (1, 9), (9, 1), (2, 3), (15, 17), (16, 16), (17, 16), (200, 120)]
FRAMES = [0, 1, 5, 1000]
JITTERS = {"none": lambda W, H: (0.0, 0.0), "subpixel": lambda W, H: (0.3 / W, -0.7 / H), "beyond": lambda W, H: (3.4 / W, -2.6 / H)}
ACCUM_REL = 2e-5        # |accum - accum64| <= (ACCUM_REL * |accum64| + CLIP_ABS * (1 + |accum64|)) / (1 - max(final_tm)): an error d in
CLIP_ABS = 1e-3         # tonemapped units becomes d / (1 - tm)^2 = d * (1 + accum) / (1 - tm) in accum. CLIP_ABS: the f32 variance clip,
                        # sigma = sqrt(m2 - m1^2) (post.wgsl:174), is off by up to ~sqrt(9 * 2^-24) in tonemapped units near sigma = 0
DISPLAY_EDGE = 1e-4     # display unorm8: +-1 only where the float64 value is this close (in [0, 1] units) to a rounding boundary


def craft(W, H, gpos, gnormal, seed):
    """Crafted RAW (f16), MOTION (f32 x 2), history ACCUM (f32 x 4) and a few G-buffer pixels: every branch of post.wgsl:187-266."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    n = W * H
    raw = rng.uniform(0.0, 2.0, (n, 4)).astype(np.float16)
    k = rng.random(n)
    raw[k < 0.05] = np.float16(65504.0)                             # f16 maximum
    raw[(k >= 0.05) & (k < 0.12)] = 0                               # zero / black
    raw[(k >= 0.12) & (k < 0.2), :3] = rng.uniform(50, 3000, ((((k >= 0.12) & (k < 0.2))).sum(), 3)).astype(np.float16)
    raw[:, 3] = 1
    hist = rng.uniform(0.0, 3.0, (n, 4)).astype(f32); hist[:, 3] = 1
    k2 = rng.random(n)
    hist[k2 < 0.1, :3] = rng.uniform(1e3, 1e5, ((k2 < 0.1).sum(), 3))          # tonemapped close to 1: near the singularity
    hist[(k2 >= 0.1) & (k2 < 0.15), :3] = 0
    ys, xs = np.divmod(np.arange(n), W)
    uv = (np.stack([xs, ys], -1).astype(f32) + f32(0.5)) / np.array([W, H], f32)
    size = np.array([W, H], f32)
    c = rng.integers(0, 12, n)
    mot = np.zeros((n, 2), f32)
    ang = rng.uniform(0, 2 * np.pi, n)
    unit = np.stack([np.cos(ang), np.sin(ang)], -1)
    speeds = {0: 0.0, 1: 0.49, 2: 0.5, 3: 0.51, 4: 1.99, 5: 2.0, 6: 2.6}
    for ci, s in speeds.items():
        m = c == ci
        if ci == 2:     # exactly 0.5 px along x (exact in f32 for power-of-two widths; otherwise the shader's own f32 rounding decides)
            mot[m] = np.array([0.5, 0.0], f32) / size
        else:
            mot[m] = (unit[m] * s / size).astype(f32)
    m = c == 7; mot[m] = -uv[m]                                      # prev_uv exactly (0, 0)
    m = c == 8; mot[m] = (f32(1) - uv[m])                            # prev_uv (1, 1) up to f32 rounding: p1 / p3 off the image
    m = c == 9; mot[m] = (rng.uniform(-3, 3, (m.sum(), 2)) / size).astype(f32)                 # taps partly off, or outside [0, 1]
    m = c == 10; mot[m] = np.array([1.5, -0.25], f32)                                          # outside
    m = c == 11; mot[m] = np.nan                                                               # NaN
    gp, gn = gpos.reshape(n, 4).copy(), gnormal.reshape(n, 4).copy()
    lonely = rng.random(n) < 0.1                                     # opposite normals and far positions: bilateral weights <= 0.001
    gn[lonely, :2] = -gn[lonely, :2]
    gp[lonely, :3] += f32(7.0) * (1 + np.arange(lonely.sum()))[:, None]
    return raw.reshape(H, W, 4), mot.reshape(H, W, 2), hist.reshape(H, W, 4), gp.reshape(H, W, 4), gn.reshape(H, W, 4)


def run_post(r, cam, W, H, fc, jitter, seed, read, write, phases, end_frame):
    """Advance r to frame fc, render the first three phases, overwrite the inputs, run POST. Returns (inputs as read back, accum, display)."""
    for _ in range(fc):
        end_frame()
    r.set_jitter(jitter)
    phases(1 | 2 | 4)
    cur, prv = fc & 1, (fc & 1) ^ 1
    raw, mot, hist, gp, gn = craft(W, H, read(GPOS, cur).view(np.float32), read(GNORMAL, cur).view(np.float32), seed)
    write(RAW, 0, raw.view(np.uint8)); write(GMOTION, 0, mot.view(np.uint8)); write(ACCUM, prv, hist.view(np.uint8))
    write(GPOS, cur, gp.view(np.uint8)); write(GNORMAL, cur, gn.view(np.uint8))
    other = read(ACCUM, cur).copy()
    phases(8)
    inp = {"gpos": read(GPOS, cur).view(np.float32), "gnormal": read(GNORMAL, cur).view(np.float32), "galbedo": read(GALBEDO, cur),
           "raw": read(RAW, 0).view(np.float16), "motion": read(GMOTION, 0).view(np.float32), "history": read(ACCUM, prv).view(np.float32)}
    # the slot rule (fill_frame_view): post reads G-buffer slot fc & 1 and accum[(fc & 1) ^ 1], writes accum[fc & 1]
    assert inp["history"].tobytes() == hist.tobytes() and inp["raw"].tobytes() == raw.tobytes()
    accum = read(ACCUM, cur)
    assert accum.tobytes() != other.tobytes() or W * H == 0
    return inp, accum.view(np.float32), read(DISPLAY, 0)


def check(inp, accum, display, W, H, fc, jitter, mis=()):
    want, disp, final_tm = R.post_f64(inp, W, H, fc, jitter, mis)
    got = accum[..., :3].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = 1.0 / np.maximum(1.0 - final_tm.max(-1), 1e-30)
    fin = np.isfinite(want).all(-1) & (cond < 1e6)
    tol = (ACCUM_REL * np.abs(want) + CLIP_ABS * (1.0 + np.abs(want))) * cond[..., None]
    bad = fin[..., None] & ~(np.abs(got - want) <= tol)
    rel = np.where(fin[..., None], np.abs(got - want) / tol, 0.0)
    assert not bad.any(), f"accum: {int(bad.any(-1).sum())} pixels out of tolerance, first at {tuple(np.argwhere(bad.any(-1))[0])}, worst {rel.max():.2e}"
    d = np.clip(disp, 0, 1) * 255.0
    q = display[..., :3].astype(np.int64)
    wq = np.floor(d + 0.5)
    edge = np.abs(d - np.floor(d) - 0.5) < DISPLAY_EDGE * 255.0
    dbad = fin[..., None] & ((np.abs(q - wq) > 1) | ((q != wq) & ~edge))
    assert not dbad.any(), f"display: {int(dbad.any(-1).sum())} pixels differ, first at {tuple(np.argwhere(dbad.any(-1))[0])}"
    return float(rel.max()), int((~fin).sum())


def _cases():
    out = [(W, H, fc, "none") for (W, H) in SIZES for fc in FRAMES]
    out += [(W, H, 5, j) for (W, H) in SIZES for j in ("subpixel", "beyond")]
    return out


def _ids():
    return [f"{W}x{H}-f{fc}-{j}" for W, H, fc, j in _cases()]


def _oracle_case(frt, orc, W, H, fc, jit):
    fs, os_ = frt.scenes.create_cornell_box(), orc.cornell()
    os_.set_bvh(fs.get("bvh2_nodes"), fs.get("bvh2_tri_index"))
    ro = os_.renderer(W, H, 1, True, 8)
    cam = frt.CameraController().build_uniform(W / H, fc, fs.num_lights)
    res = run_post(ro, cam, W, H, fc, jit, 1000 * W + H + fc, lambda b, i: ro.read(b, i), lambda b, i, d: ro.write_rows(b, i, 0, H, d),
                   lambda p: ro.render_phases(cam, p, 0, H), ro.end_frame)
    assert ro.frame_count == fc
    return fs, cam, res


@pytest.mark.parametrize("W,H,fc,jit", _cases(), ids=_ids())
def test_oracle_post_matches_float64(frt, orc, W, H, fc, jit):
    jitter = JITTERS[jit](W, H)
    _, _, (inp, accum, display) = _oracle_case(frt, orc, W, H, fc, jitter)
    worst, skipped = check(inp, accum, display, W, H, fc, jitter)
    print(f" worst accum residual / tolerance {worst:.2e}; {skipped} pixels with a non-finite or singular reference")


@pytest.fixture(scope="module")
def gpu(frt):
    if frt.lib().frt_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X (the product has no CPU path)")
    return frt


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,fc,jit", _cases(), ids=_ids())
def test_kernel_post_matches_float64_and_oracle(gpu, orc, W, H, fc, jit):
    frt = gpu
    jitter = JITTERS[jit](W, H)
    fs, cam, (oinp, oacc, odisp) = _oracle_case(frt, orc, W, H, fc, jitter)
    r = frt.Renderer(fs, W, H, max_depth=1)
    inp, accum, display = run_post(r, cam, W, H, fc, jitter, 1000 * W + H + fc, r.read_buffer, lambda b, i, d: r.write_rows(b, i, 0, H, d),
                                   lambda p: r.render_phases(cam, p), r.end_frame)
    check(inp, accum, display, W, H, fc, jitter)
    for k in inp:
        assert inp[k].tobytes() == oinp[k].tobytes(), f"post input {k} differs from the oracle's"
    assert accum.tobytes() == oacc.tobytes(), "accum differs from the oracle"
    assert display.tobytes() == odisp.tobytes(), "display differs from the oracle"
