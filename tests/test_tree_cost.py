"""tests/_tree_cost.py on hand-made quad trees whose cost is worked out here, and the null-handle refusals of the rebuild call that takes a mode
(include/frt.h: frt_renderer_rebuild_tree_ex, frt_multi_renderer_rebuild_tree_ex)."""
import numpy as np
import pytest
from _tree_cost import tree_cost, half_area, LEAF, NONE

FAR = np.float32(1.0e30)
FRT_ERR_INVALID_ARG = -1


def _node(children):
    """children: up to four (lo xyz, hi xyz, reference)."""
    q = np.full(32, FAR, np.float32)
    refs = np.full(4, NONE, np.uint32)
    for c, (lo, hi, ref) in enumerate(children):
        for a in range(3):
            q[8 * a + c] = lo[a]; q[8 * a + 4 + c] = hi[a]
        refs[c] = ref
    q[24:28] = refs.view(np.float32)
    q[28:32] = 0.0
    return q


def _leaf(first, count):
    return LEAF | (count << 24) | first


def test_half_area():
    assert half_area([0, 0, 0], [1, 2, 3]) == 1 * 2 + 2 * 3 + 3 * 1


def test_one_node_one_leaf():
    c = tree_cost(np.stack([_node([((0, 0, 0), (1, 2, 3), _leaf(0, 2))])]))
    # the root's box is its only child's: A = 11; one node, one leaf of two triangles
    assert c == {"node_term": 1.0, "leaf_term": 2.0, "root_area": 11.0, "nodes": 1, "leaves": 1}


def _two_level(order=(0, 1), stored_child_box=((0, 0, 0), (1, 1, 1))):
    kids = [(stored_child_box[0], stored_child_box[1], 1), ((1, 0, 0), (2, 1, 1), _leaf(3, 1))]
    root = _node([kids[k] for k in order])
    below = [((0, 0, 0), (0.5, 1, 1), _leaf(0, 2)), ((0.5, 0, 0), (1, 1, 1), _leaf(2, 1))]
    return np.stack([root, _node([below[k] for k in order])])


def test_two_levels():
    # root: [0,2]x[0,1]x[0,1], A = 2 + 1 + 2 = 5. Node 1: the union of its leaves, [0,1]^3, A = 3. Leaves: A = 3 (one triangle), A = 0.5 + 1 + 0.5 = 2
    # (two triangles), A = 2 (one triangle).
    c = tree_cost(_two_level())
    assert c["root_area"] == 5.0 and c["nodes"] == 2 and c["leaves"] == 3
    assert c["node_term"] == (5.0 + 3.0) / 5.0
    assert c["leaf_term"] == (3.0 * 1 + 2.0 * 2 + 2.0 * 1) / 5.0


def test_child_order_does_not_change_the_cost():
    assert tree_cost(_two_level((1, 0))) == tree_cost(_two_level((0, 1)))


def test_a_node_is_the_union_of_its_children_not_what_its_parent_stores():
    # the parent's box for node 1 is too large: the root grows (A of [-1,2]x[0,1]x[0,1] = 3 + 1 + 3 = 7), node 1 itself does not
    c = tree_cost(_two_level(stored_child_box=((-1, 0, 0), (1, 1, 1))))
    assert c["root_area"] == 7.0 and c["node_term"] == (7.0 + 3.0) / 7.0 and c["leaf_term"] == 9.0 / 7.0


def test_rebuild_with_a_mode_refuses_null_handles(frt):
    L = frt.lib()
    assert L.frt_renderer_rebuild_tree_ex(None, 1) == FRT_ERR_INVALID_ARG
    assert L.frt_multi_renderer_rebuild_tree_ex(None, 1) == FRT_ERR_INVALID_ARG
    assert L.frt_renderer_rebuild_tree_ex(None, 0) == FRT_ERR_INVALID_ARG and L.frt_renderer_rebuild_tree(None) == FRT_ERR_INVALID_ARG


def test_python_quality_names(frt):
    from frt.renderer import rebuild_mode
    assert (rebuild_mode("morton"), rebuild_mode("sah")) == (0, 1)
    with pytest.raises(ValueError):
        rebuild_mode("best")
