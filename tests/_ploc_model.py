"""A numpy model of the clustering rule of the refined tree rebuild (csrc/frt_ploc.hip; DESIGN.md section 11, "Refined rebuild"), in f32 as the
kernels compute it: every cluster i looks at i - R .. i + R (kPlocRadius = 8) for the smallest key (d, j != (i ^ 1), |i - j|, min(i, j)), d the half-area of the union
box; mutual nearest neighbours merge into the lower one's place; the array is compacted in order. Returns what bounds the device call: how many
iterations the rule takes and how high its binary tree is."""
import numpy as np

F = np.float32


def leaf_boxes(tri_lo, tri_hi):
    """Leaf j = triangles 2j and 2j + 1 (the last may hold one): (leaves, 3) lo and hi."""
    tri_lo, tri_hi = np.asarray(tri_lo, F), np.asarray(tri_hi, F)
    n = (len(tri_lo) + 1) // 2
    lo = np.minimum(tri_lo[0::2], np.concatenate([tri_lo[1::2], tri_lo[-1:]])[:n])
    hi = np.maximum(tri_hi[0::2], np.concatenate([tri_hi[1::2], tri_hi[-1:]])[:n])
    return lo, hi


def nearest(lo, hi, radius):
    n = len(lo)
    i = np.arange(n)
    best = None
    nn = np.full(n, -1, np.int64)
    for off in list(range(-radius, 0)) + list(range(1, radius + 1)):
        j = i + off
        ok = (j >= 0) & (j < n)
        jc = np.clip(j, 0, n - 1)
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.maximum(hi, hi[jc]) - np.minimum(lo, lo[jc])
            dist = (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]      # f32, the kernels' order of operations
        dist = np.where(np.isnan(dist), F(np.inf), dist).astype(np.float64)
        key = np.stack([dist, (jc != (i ^ 1)).astype(np.float64), np.abs(off) * np.ones(n), np.minimum(i, jc).astype(np.float64)], axis=1)
        if best is None:
            best = np.full((n, 4), np.inf); best[:, 0] = np.inf
            first = np.ones(n, bool)
        less = np.zeros(n, bool); tied = np.ones(n, bool)
        for k in range(4):
            less |= tied & (key[:, k] < best[:, k]); tied &= key[:, k] == best[:, k]
        take = ok & (less | (nn < 0))
        best[take] = key[take]; nn[take] = jc[take]
    return nn


def cluster(lo, hi, radius=8, max_iterations=10 ** 6):
    """(iterations, height of the binary tree in levels, a leaf = 1)"""
    lo, hi = np.asarray(lo, F).copy(), np.asarray(hi, F).copy()
    height = np.ones(len(lo), np.int64)
    it = 0
    while len(lo) > 1 and it < max_iterations:
        n = len(lo)
        nn = nearest(lo, hi, radius)
        i = np.arange(n)
        mutual = nn[nn] == i
        low, high = mutual & (i < nn), mutual & (i > nn)
        assert low.any(), "the smallest pair is chosen from both ends: every iteration merges"
        p = nn[low]
        lo[low] = np.minimum(lo[low], lo[p]); hi[low] = np.maximum(hi[low], hi[p]); height[low] = np.maximum(height[low], height[p]) + 1
        lo, hi, height = lo[~high], hi[~high], height[~high]
        it += 1
    return it, int(height.max())


def iteration_bound(leaves, factor=8):
    """csrc/frt_ploc.hip: kPlocIterFactor * ceil(log2(leaves))"""
    lg = 1
    while (1 << lg) < leaves:
        lg += 1
    return factor * lg


def chain_xs(ntris=80):
    """Triangle t at x = 2^t: every cluster's nearest neighbour is the one on its left, so one pair merges per iteration: a chain."""
    return 2.0 ** np.arange(ntris)


def chain_behind_a_row_xs(row=2048, chain=66):
    """`row` evenly spaced triangles, then a chain: enough leaves for the iteration bound to let the chain finish."""
    return np.concatenate([-0.3 * row - 10.0 + 0.3 * np.arange(row), chain_xs(chain)])


def row_boxes(xs):
    """Leaf boxes of triangles (x - 0.1, 0, -2), (x + 0.1, 0, -2), (x, 0.2, -2) as the device sees them: vertices rounded to f32, edges e = v - v0, bounds
    over v0, v0 + e1, v0 + e2."""
    x = np.asarray(xs, np.float64)
    v = [np.stack([x + dx, np.full_like(x, dy), np.full_like(x, -2.0)], axis=1).astype(F) for dx, dy in ((-0.1, 0.0), (0.1, 0.0), (0.0, 0.2))]
    p = [v[0], v[0] + (v[1] - v[0]), v[0] + (v[2] - v[0])]
    return leaf_boxes(np.minimum(p[0], np.minimum(p[1], p[2])), np.maximum(p[0], np.maximum(p[1], p[2])))
