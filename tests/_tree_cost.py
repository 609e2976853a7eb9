"""A numpy surface-area cost of a quad tree, given the bytes of selectors 10 (quad nodes) and 13 (triangle slots) of frt_scene_get /
frt_renderer_read_scene (layouts: tests/_tree_check.py). A node's box is the union of its live child boxes; A is the half-area dx*dy + dy*dz + dz*dx.
node_term = sum over nodes of A(node) / A(root): the expected number of nodes a random ray through the root's box visits. leaf_term = sum over leaf
children of A(leaf box) / A(root) * triangle count: the expected number of triangle tests. Both are summed exactly (math.fsum), so two trees over
the same leaves have the same leaf_term to the last bit whatever their node order."""
import math
import numpy as np

LEAF, NONE = 0x80000000, 0xFFFFFFFF


def half_area(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def tree_cost(nodes, slots=None):
    """nodes: (n, 32) float32 quad nodes; slots is accepted for symmetry with check_tree and not needed (leaf boxes are stored in the nodes).
    Returns {"node_term", "leaf_term", "root_area", "nodes", "leaves"}."""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 32)
    refs = nodes[:, 24:28].view(np.uint32)
    live = refs != NONE
    leaf = live & ((refs & LEAF) != 0)
    lo = np.stack([nodes[:, 0:4], nodes[:, 8:12], nodes[:, 16:20]], axis=2).astype(np.float64)      # (n, child, axis)
    hi = np.stack([nodes[:, 4:8], nodes[:, 12:16], nodes[:, 20:24]], axis=2).astype(np.float64)
    nlo = np.where(live[:, :, None], lo, np.inf).min(axis=1)
    nhi = np.where(live[:, :, None], hi, -np.inf).max(axis=1)
    node_area = half_area(nlo, nhi)
    root = float(node_area[0])
    count = ((refs >> 24) & 0x7F).astype(np.float64)
    leaf_area = half_area(lo, hi)[leaf] * count[leaf]
    return {"node_term": math.fsum(node_area.tolist()) / root, "leaf_term": math.fsum(leaf_area.tolist()) / root, "root_area": root,
            "nodes": int(len(nodes)), "leaves": int(leaf.sum())}
