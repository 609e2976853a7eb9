"""The workgroup -> (region, offset) map of continue_kernel (csrc/frt_kernels.hpp: cont_region_slots) on the host: for random fills of the regions
of a continuation queue, the grid the launch uses visits every parked slot exactly once and no slot beyond a region's fill, whatever the
capacity, the number of regions and the surplus of the grid. CPU-only (tests/hostcheck/frt_region_map_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
THREADS = 256


@pytest.fixture(scope="module")
def rmap(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("region_map_check") / "libfrt_region_map_check.so")
    flags = "-O2 -std=c++17 -fPIC --cuda-host-only -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function".split()
    subprocess.run([HIPCC] + flags + ["-x", "hip", os.path.join(ROOT, "tests", "hostcheck", "frt_region_map_check.cpp"), "-shared", "-o", out], check=True)
    L = C.CDLL(out)
    L.rm_grid_blocks.restype = C.c_uint32; L.rm_grid_blocks.argtypes = [C.c_uint32] * 3
    L.rm_walk.restype = C.c_uint32; L.rm_walk.argtypes = [C.c_uint32] * 4 + [C.c_void_p] * 2
    return L


# capacities: whole rows of every region, a region of less than a wave, fewer slots than regions, slots that no region owns (capacity % nsub != 0)
@pytest.mark.parametrize("nsub", [1, 2, 16, 64, 256])
@pytest.mark.parametrize("capacity", [1, 100, 1024, 4096, 16384 + 77, 518400])
def test_every_parked_slot_is_visited_exactly_once(rmap, nsub, capacity):
    rng = np.random.default_rng(1000 * nsub + capacity % 997)
    rcap = capacity // nsub
    blocks = rmap.rm_grid_blocks(capacity, nsub, THREADS)
    assert blocks == nsub * ((rcap + THREADS - 1) // THREADS)
    for trial in range(4):
        # empty regions, partly filled ones, exactly full ones and counters that ran past the region's capacity
        counts = rng.integers(0, 2 * rcap + 2, nsub).astype(np.uint32)
        counts[rng.random(nsub) < 0.2] = 0
        counts[rng.random(nsub) < 0.1] = rcap
        surplus = (0, 1, 3 * nsub + 5, 4 * blocks)[trial]      # (the spatial continuation grids cover more than the capacity)
        visits = np.zeros(max(capacity, 1), np.uint32)
        staying = rmap.rm_walk(capacity, nsub, THREADS, blocks + surplus, counts.ctypes.data, visits.ctypes.data)
        want = np.zeros_like(visits)
        n = np.minimum(counts, rcap)
        for g in range(nsub):
            want[g * rcap:g * rcap + n[g]] = 1
        assert np.array_equal(visits, want), (nsub, capacity, trial)
        assert staying == int(((n + THREADS - 1) // THREADS).sum())
        # the workgroups that stay are those of the lowest offsets: they lie in the front of the grid (nsub x the fullest region's rows)
        assert staying <= nsub * ((int(n.max(initial=0)) + THREADS - 1) // THREADS)
