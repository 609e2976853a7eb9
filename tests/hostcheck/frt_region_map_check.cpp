// TEST INFRASTRUCTURE ONLY — not linked into libfrt.so.
// The workgroup -> (region, offset) map of continue_kernel (csrc/frt_kernels.hpp: cont_region_slots, cont_grid_blocks) on the host, walked the way
// the kernel walks it: every workgroup of the grid the launch would use, every lane, the region's fill clamped to the region's capacity.
// tests/test_regional_queues.py checks that every parked slot is visited exactly once and none beyond a region's fill.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_kernels.hpp"

using namespace frt;

extern "C" {
uint32_t rm_grid_blocks(uint32_t capacity, uint32_t nsub, uint32_t threads) { return cont_grid_blocks(capacity, nsub, threads); }

// visits[slot] += 1 for every queue slot a lane of a grid of `blocks` workgroups would load; returns the number of workgroups that stay
// (those whose offset lies below their region's fill). counts[g]: what region g's counter holds (it may run past the region's capacity).
uint32_t rm_walk(uint32_t capacity, uint32_t nsub, uint32_t threads, uint32_t blocks, const uint32_t* counts, uint32_t* visits) {
    const uint32_t rcap = capacity / nsub;
    uint32_t staying = 0;
    for (uint32_t wg = 0; wg < blocks; ++wg) {
        const RegionSlots m = cont_region_slots(wg, nsub, threads);
        const uint32_t filled = counts[m.region], n = filled < rcap ? filled : rcap;
        if (m.offset >= n) continue;
        ++staying;
        for (uint32_t t = 0; t < threads; ++t)
            if (m.offset + t < n) visits[m.region * rcap + m.offset + t] += 1u;
    }
    return staying;
}
}
