"""tests/_tree_check.py proven on the host: it accepts the host-built quad trees of the Cornell Box, the ReSTIR scene and the 82k-triangle blob
(frt_scene_get selectors 10 and 13) and computes the stack need frt_scene_tree_stats reports; it rejects a dropped triangle, a duplicated slot, a box
shrunk by one ulp and a child index not greater than its parent."""
import numpy as np
import pytest
from _tree_check import check_tree, TreeError, LEAF, NONE


def _scene(frt, orc, which):
    import _scenes
    if which == "cornell":
        return frt.scenes.create_cornell_box()
    if which == "restir":
        return frt.scenes.create_restir_scene()
    return _scenes.bumpy_sphere_in_box(frt, orc, subdiv=6)[0]


@pytest.mark.parametrize("which", ["cornell", "restir", "blob82k"])
def test_validator_accepts_the_host_built_trees(frt, orc, which):
    fs = _scene(frt, orc, which)
    got = check_tree(fs.get("quad_nodes"), fs.get("tri_slots"))
    st = fs.tree_stats()
    assert got["quad_nodes"] == st["quad_nodes"]
    assert got["quad_stack_need"] == st["quad_stack_need"]
    assert got["quad_levels"] >= 1


def _first(refs, pred):
    for i in range(len(refs)):
        for c in range(4):
            if pred(i, c, int(refs[i, c])):
                return i, c
    raise AssertionError("the scene has no such reference")


@pytest.fixture(scope="module")
def cornell_tree(frt):
    fs = frt.scenes.create_cornell_box()
    return fs.get("quad_nodes").copy(), fs.get("tri_slots").copy()


def test_validator_rejects_a_dropped_triangle(cornell_tree):
    nodes, slots = (a.copy() for a in cornell_tree)
    refs = nodes[:, 24:28].view(np.uint32)
    i, c = _first(refs, lambda i, c, r: r != NONE and (r & LEAF) and ((r >> 24) & 0x7F) == 2)
    refs[i, c] = LEAF | (1 << 24) | (int(refs[i, c]) & 0xFFFFFF)      # the leaf keeps its first triangle only
    with pytest.raises(TreeError, match="in no leaf"):
        check_tree(nodes, slots)


def test_validator_rejects_a_duplicated_slot(cornell_tree):
    nodes, slots = (a.copy() for a in cornell_tree)
    refs = nodes[:, 24:28].view(np.uint32)
    i, c = _first(refs, lambda i, c, r: r != NONE and (r & LEAF) and (r & 0xFFFFFF) >= 1 and ((r >> 24) & 0x7F) == 1)
    refs[i, c] = LEAF | (2 << 24) | ((int(refs[i, c]) & 0xFFFFFF) - 1)  # now also holds the slot before it, which another leaf has
    with pytest.raises(TreeError, match="leaves"):
        check_tree(nodes, slots)
    nodes, slots = (a.copy() for a in cornell_tree)
    slots[1, 3] = slots[0, 3]                                           # two slots with one triangle id
    with pytest.raises(TreeError, match="permutation"):
        check_tree(nodes, slots)


@pytest.mark.parametrize("kind", ["leaf", "inner"])
def test_validator_rejects_a_box_shrunk_by_one_ulp(cornell_tree, kind):
    nodes, slots = (a.copy() for a in cornell_tree)
    refs = nodes[:, 24:28].view(np.uint32)
    want_leaf = kind == "leaf"
    i, c = _first(refs, lambda i, c, r: r != NONE and bool(r & LEAF) == want_leaf)
    nodes[i, 4 + c] = np.nextafter(nodes[i, 4 + c], np.float32(-np.inf))   # hi.x of that child, one ulp down
    with pytest.raises(TreeError, match="padded union"):
        check_tree(nodes, slots)
    nodes, slots = (a.copy() for a in cornell_tree)
    nodes[i, 16 + c] = np.nextafter(nodes[i, 16 + c], np.float32(np.inf))  # lo.z, one ulp up
    with pytest.raises(TreeError, match="padded union"):
        check_tree(nodes, slots)


def test_validator_rejects_a_child_index_not_greater_than_its_parent(cornell_tree):
    nodes, slots = (a.copy() for a in cornell_tree)
    refs = nodes[:, 24:28].view(np.uint32)
    i, c = _first(refs, lambda i, c, r: i >= 1 and r != NONE and not (r & LEAF))
    refs[i, c] = i
    with pytest.raises(TreeError, match="not greater than its parent"):
        check_tree(nodes, slots)


def test_validator_rejects_a_malformed_empty_slot(cornell_tree):
    nodes, slots = (a.copy() for a in cornell_tree)
    refs = nodes[:, 24:28].view(np.uint32)
    i, c = _first(refs, lambda i, c, r: r == NONE)
    nodes[i, 8 + c] = 0.0
    with pytest.raises(TreeError, match="empty slot"):
        check_tree(nodes, slots)
