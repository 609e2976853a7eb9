// frt_rebuild.hpp — device side of frt_renderer_rebuild_tree ("Rebuild"): a new quad tree over the triangle slots as they are on the
// device, built into a second set of buffers. Morton keys of the centroids, rocPRIM's radix sort, Karras's binary radix tree over leaves of two
// adjacent sorted slots, a topological fold into quad nodes under build_quad_nodes's stack rule (frt_bvh.cpp: `fits`), breadth-first numbering by a
// per-level scan, boxes by the existing refit kernel. Every index is assigned by a sort or a scan: two rebuilds of one device state give the same bytes.
// The refined mode (FRT_REBUILD_SAH, "Refined rebuild") shares all of it but the binary topology (frt_ploc.hip) and the order of the fold.
#pragma once
#include "frt_refit.hpp"
#include <vector>

namespace frt {

// Scratch of the rebuild, one allocation made at the first call and kept (frt_rebuild.hip: rebuild_reserve): the keys (2 x 8 B per triangle), the
// sort's and the scan's temporary storage, and per binary inner node (one per leaf pair, less one) 11 words: topology (2), level, height, two
// frontiers with their `used` (4), child count, scan, stack need.
// The small results (RebuildScratch::words): [0..2] min and [3..5] max of the centroids as ordered bits, [6] the size of the next frontier,
// [8 + L] whether the binary tree has inner nodes on level L; the refined mode's words follow: the live cluster count and the number of inner nodes
// made so far, each in two words that iterations of even and odd number read and write alternately (a kernel never writes a word it reads), the
// iterations run and whether the tail kernel stopped at its bound.
enum { W_MIN = 0, W_MAX = 3, W_NEXT = 6, W_FLAGS = 8, kMaxBinaryLevels = 64, W_PCOUNT = W_FLAGS + kMaxBinaryLevels + 1, W_PNODES = W_PCOUNT + 2,
       W_PITERS = W_PNODES + 2, W_PFAIL = W_PITERS + 1, kRebuildWords = W_FLAGS + kMaxBinaryLevels + 8 };
static_assert(W_PFAIL < kRebuildWords, "the refined mode's words lie inside the words buffer");

// Extra scratch of the refined mode (frt_ploc.hip), one allocation: two cluster arrays (box as six planes of `cap` floats, id), the nearest
// neighbour, the packed merge / keep flags and their scan (8 B each), the scan's temporary storage, and one box (6 floats) per binary inner node.
struct PlocScratch {
    void* base = nullptr; size_t bytes = 0;
    uint32_t cap = 0;                                  // leaves the arrays hold
    float* cbox[2] = {nullptr, nullptr}; uint32_t* cid[2] = {nullptr, nullptr};
    uint32_t* nn = nullptr;
    unsigned long long* flag = nullptr; unsigned long long* scan = nullptr;
    void* scan_tmp = nullptr; size_t scan_bytes = 0;
    float* nbox = nullptr;
};

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
    PlocScratch ploc;               // the refined mode's own allocation (ploc_reserve), made at the first FRT_REBUILD_SAH call
};

// What rebuild_tree hands to the caller for a new set of buffers: the caller allocates `nodes` with room for rebuild_max_nodes(num_tris) quad nodes,
// `tris` and `slot_of` as large as the current ones.
struct RebuildTarget { float4* tris; float4* nodes; uint32_t* slot_of; };
struct RebuildResult {
    uint32_t num_nodes = 0, stack_need = 0;
    uint32_t origin = 1;               // 1 the Morton radix tree, 2 the refined tree (frt.h: frt_renderer_tree_stats)
    uint32_t iterations = 0;           // refined mode: clustering iterations run
    uint32_t fell_back = 0;            // refined mode: 0 no; the Morton tree was built instead because 1 the iteration bound was passed, 2 the refined tree does not fit the stack
    std::vector<uint32_t> levels;      // level L = quad nodes [levels[L], levels[L + 1])
};

inline uint32_t rebuild_max_nodes(uint32_t num_tris) { const uint32_t leaves = (num_tris + 1u) / 2u; return leaves > 1u ? leaves - 1u : 1u; }
// Allocates the scratch for a scene of `num_tris` triangles (nothing when it is already large enough).
hipError_t rebuild_reserve(RebuildScratch& s, uint32_t num_tris);
void rebuild_release(RebuildScratch& s);
// Builds the new tree of `cur` (tris, num_tris; `slot_of` its id -> slot table) into `out` on `stream`; waits for the stream (level counts and the
// stack need come back to the host). `ext` is the renderer's scene-extent word. Nothing of `cur` is written. hipSuccess with res.num_nodes == 0:
// the tree could not be numbered inside its buffers (corrupt input); the caller must not swap.
// `mode`: FRT_REBUILD_MORTON (0) or FRT_REBUILD_SAH (1; ploc_reserve first). The refined mode falls back to the Morton topology inside the call when
// its tree does not fit the traversal stack or its iteration bound is passed: res.origin tells which tree `out` holds.
hipError_t rebuild_tree(RebuildScratch& s, const SceneView& cur, const uint32_t* slot_of, const RebuildTarget& out, unsigned int* ext, hipStream_t stream, RebuildResult& res, uint32_t mode = 0u);
// The small results, on the host, once everything enqueued so far has run.
hipError_t rebuild_fetch_words(RebuildScratch& s, hipStream_t stream);

// Refined mode (frt_ploc.hip). ploc_reserve: the extra scratch for `num_tris` triangles (nothing when large enough; rebuild_release frees it).
// ploc_topology: the binary tree over the leaves of `tris` (leaf j = slots 2j, 2j + 1) by parallel locally-ordered clustering, into s.left / s.right
// with each inner node's box in s.ploc.nbox; the root is inner node leaves - 2, the last one made. Waits for the stream. `ok` is false when
// the iteration bound was passed (the topology is then incomplete and must not be used).
hipError_t ploc_reserve(RebuildScratch& s, uint32_t num_tris);
hipError_t ploc_topology(RebuildScratch& s, const float4* tris, uint32_t num_tris, hipStream_t stream, uint32_t& iterations, bool& ok);

} // namespace frt
