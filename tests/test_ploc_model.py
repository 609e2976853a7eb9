"""The clustering rule of the refined tree rebuild on inputs whose outcome is known (tests/_ploc_model.py): what its tie rule does to fully tied
input, and the two scenes tests/test_tree_rebuild_sah_gpu.py uses to reach the two fallbacks of the device call."""
import numpy as np
from _ploc_model import cluster, iteration_bound, row_boxes as _row, chain_xs, chain_behind_a_row_xs


def test_fully_tied_input_merges_even_odd_pairs_everywhere():
    # 301 coincident triangles, 151 leaves: every distance is equal, the i ^ 1 term pairs (0, 1), (2, 3), ...: the array halves every iteration
    it, height = cluster(*_row(np.zeros(301)))
    assert (it, height) == (8, 9)


def test_evenly_spaced_input_stays_shallow():
    it, height = cluster(*_row(0.3 * np.arange(301)))
    print(f"151 evenly spaced leaves: {it} iterations, height {height}")
    assert it <= 16 and height <= 11 and it < iteration_bound(151)


def test_geometric_spacing_is_a_chain():
    # triangles at x = 2^t: every cluster's nearest neighbour is on its left, one pair merges per iteration. 40 leaves are inside the iteration bound
    # (48) and too deep for the stack (a binary chain of h levels needs h - 1 entries however it is folded); 60 leaves pass the bound (still 48).
    assert cluster(*_row(chain_xs(80))) == (39, 40) and iteration_bound(40) == 48
    assert cluster(*_row(chain_xs(120))) == (59, 60) and iteration_bound(60) == 48


def test_a_chain_behind_a_balanced_part_is_inside_the_iteration_bound_and_too_deep_for_the_stack():
    # 2048 evenly spaced triangles, then 66 at x = 2^t: 1057 leaves, bound 88, and more leaves than the tail kernel takes (1024). The chain still merges one pair per iteration, so the tree is
    # finished in time, and a binary chain of h levels needs h - 1 stack entries however it is folded (a quad node that swallows three
    # chain levels pushes three entries): more than 31.
    xs = chain_behind_a_row_xs()
    it, height = cluster(*_row(xs))
    print(f"{(len(xs) + 1) // 2} leaves: {it} iterations (bound {iteration_bound((len(xs) + 1) // 2)}), height {height}")
    assert it + 4 <= iteration_bound((len(xs) + 1) // 2)      # (with room for a last-bit difference in the even part)
    assert height - 1 > 31
