"""A numpy validator of a quad tree, given the bytes of selectors 10 (quad nodes) and 13 (triangle slots) of frt_scene_get / frt_renderer_read_scene.
It knows the layouts (csrc/frt_bvh.cpp: build_quad_nodes; csrc/frt_scene.hpp: TriSlot) and DESIGN.md section 11's definition of a box, and nothing of
how a tree was made: whatever passes is a tree the kernels can walk and the refit kernel would leave unchanged."""
import numpy as np

LEAF, NONE = 0x80000000, 0xFFFFFFFF
FAR = np.float32(1.0e30)


class TreeError(AssertionError):
    pass


def _need(cond, msg):
    if not cond:
        raise TreeError(msg)


def check_tree(nodes, slots):
    """nodes: (n, 32) float32 (lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.z[4], hi.z[4], reference[4], unused[4]); slots: (N, 12) float32.
    Raises TreeError on the first violation; returns {"quad_nodes", "quad_stack_need", "quad_levels"} computed from the tree alone."""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 32)
    slots = np.ascontiguousarray(slots, np.float32).reshape(-1, 12)
    n, N = len(nodes), len(slots)
    _need(n >= 1 and N >= 1, "empty tree")
    refs = nodes[:, 24:28].view(np.uint32)
    # ids form a permutation
    ids = slots[:, 3].view(np.uint32)
    _need(np.array_equal(np.sort(ids), np.arange(N, dtype=np.uint32)), "triangle ids are not a permutation of 0 .. N - 1")
    # bounds of the triangles the intersector sees, in f32, and the pad
    v0, v1, v2 = slots[:, 0:3], slots[:, 0:3] + slots[:, 4:7], slots[:, 0:3] + slots[:, 8:11]
    slo = np.minimum(v0, np.minimum(v1, v2)); shi = np.maximum(v0, np.maximum(v1, v2))
    ext = max(np.float32(np.abs(slo).max()), np.float32(np.abs(shi).max()))
    pad = np.float32(1e-4) * max(ext, np.float32(1.0))
    # leaves: every slot referenced by exactly one leaf, ranges disjoint and covering
    is_none = refs == NONE
    is_leaf = ((refs & LEAF) != 0) & ~is_none
    is_inner = ~is_none & ~is_leaf
    first = (refs & 0xFFFFFF).astype(np.int64); count = ((refs >> 24) & 0x7F).astype(np.int64)
    _need(bool((count[is_leaf] >= 1).all()), "a leaf without triangles")
    _need(bool((first[is_leaf] + count[is_leaf] <= N).all()), "a leaf reaches beyond the triangle slots")
    cover = np.zeros(N + 1, np.int64)
    np.add.at(cover, first[is_leaf], 1); np.add.at(cover, first[is_leaf] + count[is_leaf], -1)
    cover = np.cumsum(cover)[:N]
    _need(bool((cover >= 1).all()), f"slot {int(np.argmin(cover))} is in no leaf")
    _need(bool((cover <= 1).all()), f"slot {int(np.argmax(cover))} is in {int(cover.max())} leaves")
    # inner references: greater than their parent, inside the array, every node but the root referenced exactly once
    parent_of = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], refs.shape)
    child = refs[is_inner].astype(np.int64)
    _need(bool((child < n).all()), "a child index beyond the node array")
    _need(bool((child > parent_of[is_inner]).all()), "a child index not greater than its parent")
    seen = np.bincount(child, minlength=n)
    _need(seen[0] == 0 and bool((seen[1:] == 1).all()), "a node is not referenced exactly once")
    _need(bool((~is_none).any(axis=1).all()), "a node without children")
    # levels: contiguous ranges in index order; the root's inner children are 1 .. k
    level = np.zeros(n, np.int64)
    for i in range(n):
        for c in range(4):
            if is_inner[i, c]:
                level[refs[i, c]] = level[i] + 1
    _need(bool((np.diff(level) >= 0).all()) and bool((np.diff(level) <= 1).all()), "levels are not contiguous index ranges")
    root_kids = np.sort(refs[0][is_inner[0]].astype(np.int64))
    _need(np.array_equal(root_kids, np.arange(1, len(root_kids) + 1)), "the root's children are not nodes 1 .. k")
    # boxes (bottom-up: children have larger indices) and the stack need
    lo = np.stack([nodes[:, 0:4], nodes[:, 8:12], nodes[:, 16:20]], axis=1)           # (n, axis, child)
    hi = np.stack([nodes[:, 4:8], nodes[:, 12:16], nodes[:, 20:24]], axis=1)
    need = np.zeros(n, np.int64)
    inf = np.float32(np.inf)
    for i in range(n - 1, -1, -1):
        kids, deepest = 0, 0
        for c in range(4):
            if is_none[i, c]:
                _need(bool((lo[i, :, c] == FAR).all()) and bool((hi[i, :, c] == FAR).all()), f"node {i} child {c}: an empty slot without the far-away point box")
                continue
            kids += 1
            if is_leaf[i, c]:
                a, b = first[i, c], first[i, c] + count[i, c]
                wlo = slo[a:b].min(axis=0) - pad; whi = shi[a:b].max(axis=0) + pad
            else:
                k = int(refs[i, c]); live = ~is_none[k]
                wlo = np.where(live[None, :], lo[k], inf).min(axis=1); whi = np.where(live[None, :], hi[k], -inf).max(axis=1)
                deepest = max(deepest, int(need[k]))
            _need(bool((lo[i, :, c] == wlo.astype(np.float32)).all()) and bool((hi[i, :, c] == whi.astype(np.float32)).all()),
                  f"node {i} child {c}: box {lo[i, :, c]} .. {hi[i, :, c]} is not the padded union {wlo} .. {whi}")
        need[i] = kids - 1 + deepest
    return {"quad_nodes": n, "quad_stack_need": int(need[0]), "quad_levels": int(level[-1]) + 1}
