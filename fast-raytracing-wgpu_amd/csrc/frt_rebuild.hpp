// frt_rebuild.hpp — device side of frt_renderer_rebuild_tree ("Rebuild"): a new quad tree over the triangle slots as they are on the
// device, built into a second set of buffers. Morton keys of the centroids, rocPRIM's radix sort, Karras's binary radix tree over leaves of two
// adjacent sorted slots, a topological fold into quad nodes under build_quad_nodes's stack rule (frt_bvh.cpp: `fits`), breadth-first numbering by a
// per-level scan, boxes by the existing refit kernel. Every index is assigned by a sort or a scan: two rebuilds of one device state give the same bytes.
#pragma once
#include "frt_refit.hpp"
#include <vector>

namespace frt {

// Scratch of the rebuild, one allocation made at the first call and kept (frt_rebuild.hip: rebuild_reserve): the keys (2 x 8 B per triangle), the
// sort's and the scan's temporary storage, and per binary inner node (one per leaf pair, less one) 11 words: topology (2), level, height, two
// frontiers with their `used` (4), child count, scan, stack need.
struct RebuildScratch {
    void* base = nullptr; size_t bytes = 0;
    uint32_t cap_tris = 0, cap_inner = 0;
    unsigned long long* keys[2] = {nullptr, nullptr};
    void* sort_tmp = nullptr; size_t sort_bytes = 0;
    void* scan_tmp = nullptr; size_t scan_bytes = 0;
    uint32_t* left = nullptr; uint32_t* right = nullptr; uint32_t* level = nullptr; uint32_t* height = nullptr;
    uint32_t* front[2] = {nullptr, nullptr}; uint32_t* used[2] = {nullptr, nullptr};
    uint32_t* cnt = nullptr; uint32_t* off = nullptr; uint32_t* need = nullptr;
    uint32_t* words = nullptr;      // kRebuildWords small results (frt_rebuild.hip)
    uint32_t* h_words = nullptr;    // their pinned host copy
};

// What rebuild_tree hands to the caller for a new set of buffers: the caller allocates `nodes` with room for rebuild_max_nodes(num_tris) quad nodes,
// `tris` and `slot_of` as large as the current ones.
struct RebuildTarget { float4* tris; float4* nodes; uint32_t* slot_of; };
struct RebuildResult {
    uint32_t num_nodes = 0, stack_need = 0;
    std::vector<uint32_t> levels;      // level L = quad nodes [levels[L], levels[L + 1])
};

inline uint32_t rebuild_max_nodes(uint32_t num_tris) { const uint32_t leaves = (num_tris + 1u) / 2u; return leaves > 1u ? leaves - 1u : 1u; }
// Allocates the scratch for a scene of `num_tris` triangles (nothing when it is already large enough).
hipError_t rebuild_reserve(RebuildScratch& s, uint32_t num_tris);
void rebuild_release(RebuildScratch& s);
// Builds the new tree of `cur` (tris, num_tris; `slot_of` its id -> slot table) into `out` on `stream`; waits for the stream (level counts and the
// stack need come back to the host). `ext` is the renderer's scene-extent word. Nothing of `cur` is written. hipSuccess with res.num_nodes == 0:
// the tree could not be numbered inside its buffers (corrupt input); the caller must not swap.
hipError_t rebuild_tree(RebuildScratch& s, const SceneView& cur, const uint32_t* slot_of, const RebuildTarget& out, unsigned int* ext, hipStream_t stream, RebuildResult& res);

} // namespace frt
