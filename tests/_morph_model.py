"""What the morph-target tests share (include/frt.h: frt_scene_set_mesh_morph_targets, frt_scene_set_mesh_morph_weights; DESIGN.md section 11, "Morph
targets"): the float32 numpy model of the contract, written as elementwise * and + in target order, and deterministic synthetic targets and weights."""
import numpy as np

F = np.float32
TARGET_COUNTS = (1, 3, 70)


def morph_model(base, deltas, weights):
    """out[:, r] = ((b[:, r] + w_0 d_0[:, r]) + w_1 d_1[:, r]) + ... in target order, every term evaluated; out.w = b.w."""
    out = np.ascontiguousarray(base, F).copy()
    d, w = np.ascontiguousarray(deltas, F), np.ascontiguousarray(weights, F)
    assert d.ndim == 3 and d.shape[1:] == (len(out), 3) and w.shape == (d.shape[0],)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(d.shape[0]):
            for r in range(3):
                out[:, r] = out[:, r] + F(w[t]) * d[t, :, r]
    assert out.dtype == F
    return out


def make_targets(n, ntargets, seed=0):
    """[ntargets, n, 3] float32 deltas for a mesh of n >= 2 vertices, small against a unit-sized mesh (|d| < 0.06). The last target of several is all zeros; vertex
    1 has a zero delta in every target. (A single target is not zeroed: it would morph nothing.)"""
    rng = np.random.default_rng(2000 * ntargets + n + seed)
    d = (0.12 * (rng.random((ntargets, n, 3)) - 0.5)).astype(F)
    if ntargets > 1:
        d[-1] = 0.0
    d[:, 1, :] = 0.0
    return d


def make_weights(ntargets, phase=0.0):
    """[ntargets] float32 weights. From three targets on: an exact 0 (target 0), a negative weight (target 1) and one above 1 (target 2); a single
    target gets 1.25 or, at an odd phase step, -0.5, two targets get (0, 1.5) or (0, -0.5)."""
    rng = np.random.default_rng(11 * ntargets + int(round(100 * phase)))
    w = rng.random(ntargets).astype(F)
    odd = int(round(10 * phase)) % 2 == 1
    if ntargets >= 3:
        w[0], w[1], w[2] = 0.0, -0.375 - F(phase) * F(0.1), 1.5 + F(phase) * F(0.1)
    elif ntargets == 2:
        w[0], w[1] = 0.0, (-0.5 if odd else 1.5)
    else:
        w[0] = -0.5 if odd else 1.25
    return w


def overflowing_weights(n, ntargets):
    """(deltas, weights), all finite, whose weighted sum carries coordinates past the largest float: make_targets' deltas times 2e37 (up to 1.2e36 in
    size) under weights of 1e3, so that a single term reaches 1.2e39."""
    d = (make_targets(n, ntargets) * F(2.0e37)).astype(F)
    w = np.full(ntargets, 1.0e3, F)
    assert np.isfinite(d).all() and np.isfinite(w).all()
    return d, w
