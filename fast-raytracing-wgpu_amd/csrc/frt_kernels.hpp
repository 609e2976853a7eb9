// frt_kernels.hpp — host-callable launch entry points of frt_kernels.hip.
#pragma once
#include "frt_mono.hpp"
#include <algorithm>

namespace frt {
// How to launch a traced stage (1 = T-trace, 2 = spatial + shade): pixel kernel cut at cuts[0] + one continuation launch per further
// segment. The two word buffers are used alternately by the segments (the second one only exists when there are two cuts or more);
// every segment has its OWN counter (counts[0 .. ncuts], zero before the stage runs), so a buffer that is written again two launches
// later starts from slot 0. `zero_counts`: the counter set of this stage's NEXT launch, cleared in passing by the pixel kernel.
// A queue is cut into `nsub` regions (frt_mono.hpp: ContQueue): region g of segment k counts in counts[g * kRegionStride + k], so a region's
// counters fill one 128-byte line of their own and a set is nsub lines.
static constexpr int kMaxCuts = 4;
static constexpr uint32_t kMaxRegions = 256u;
enum { kWalkQuad = 0, kWalkWide = 2, kWalkWideLds = 3, kWalkQuadWg = 4 };      // (1 = the quad walk with the voting loop: TraceLaunch::vote; kWalkQuadWg: the quad walk, a workgroup's rays re-dealt to dense direction-sorted waves: frt_kernels.hip: wg_trace)
#ifndef FRT_EXPERIMENTS
#define FRT_EXPERIMENTS 0
#endif
struct TraceLaunch {
    uint32_t ncuts; uint32_t cuts[kMaxCuts]; uint32_t* qwords[2]; uint32_t* counts;
    uint32_t capacity, capacity_odd, grid_min_slots;   // capacity_odd: slots of qwords[1] (the odd segments: far fewer paths get that far); grid_min_slots: the continuation grids cover at least this many slots
    uint32_t* overflow;
    uint32_t* zero_counts;
    uint32_t nsub;  // regions of every queue and of the ray counters: a power of two <= kMaxRegions (1: the kernel families that read one counter)
    bool vote;      // the kernels whose BVH walk votes for its next step (frt_trace.hpp: trace4<ANY, VOTE>): scenes with a deep tree
    uint32_t walk;  // which tree the traced kernels walk: kWalkQuad (trace4; `vote` picks its loop), kWalkWide (trace8, nodes read from HBM), kWalkWideLds (trace8, the whole 8-wide tree copied into every workgroup's LDS: wide_lds_bytes of dynamic LDS)
    uint32_t wide_lds_bytes;
    uint32_t wg_rows;   // rows of a quad-walk workgroup's dynamic LDS: the quad tree's stack need + the shared row (walk_lds_plan below; kWalkQuadWg adds its exchange rows)
    uint32_t lds_budget;   // bytes of LDS a traced workgroup may use (traced_lds_budget below); 0 = the default
#if FRT_EXPERIMENTS
    // lib/libfrt_exp.so only (csrc/experiments/frt_experiment_kernels.hpp): the measured-and-not-kept kernel designs
    uint32_t* tile_state;   // the stage's sweep-direction state (TileOrder) or null = tile rows top to bottom
    bool wavefront; uint32_t* wf_words[2]; uint32_t* wf_items[2]; uint32_t* wf_hits;   // ray-level wavefront (wf_*_kernel); counts = its 96-word counter block
    bool stream; uint32_t shade_min, slice;   // single cut: stream_kernel (resumable traversal + lane refill); shade when >= shade_min lanes wait
    bool refill; uint32_t refill_min;   // single cut: bounce_kernel (lane refill) instead of the continuation launches; refill when >= refill_min lanes are free
    bool resident; uint32_t res_nodes; bool res_tris; uint32_t num_cus; uint32_t res_batch;   // resident_*_kernel: BVH cached in LDS, persistent workgroups; res_batch: 0 = chosen from the tile count
    uint32_t* work;   // 2 x (1 + kMaxCuts) words: {next, ticket} of the pixel launch, then of each continuation launch; zero between launches
#endif
};
// The top of the quad tree — nodes 0 .. n - 1; the tree is numbered breadth-first — copied into the workgroup's LDS behind the shared words of the row
// that follows the stack rows, 16 bytes per lane and coalesced. The
// node steps of a walk whose whole wave is among these nodes read them there. Call before the workgroup's first barrier; null for n = 0.
// Without `n`: the five nodes that fit the shared row itself (the ray-query kernels), none for a smaller tree.
static constexpr uint32_t kLdsSharedWords = 32u;      // words of the shared row in front of the node copy (ray-count sums, reservation scratch): 128 bytes
__device__ __forceinline__ const uint32_t* stage_top_nodes(const SceneView& sc, uint32_t* s_cnt, uint32_t n) {
    uint4* const s_top = reinterpret_cast<uint4*>(s_cnt + kLdsSharedWords);      // (128-byte aligned)
    if (n == 0u) return nullptr;
    const uint4* const src = reinterpret_cast<const uint4*>(sc.nodes4);
    for (uint32_t i = threadIdx.x; i < n * 8u; i += blockDim.x) s_top[i] = src[i];
    return reinterpret_cast<const uint32_t*>(s_top);
}
__device__ __forceinline__ const uint32_t* stage_top_nodes(const SceneView& sc, uint32_t* s_cnt) {
    return stage_top_nodes(sc, s_cnt, sc.num_nodes4 < (uint32_t)kLdsTopNodes ? 0u : (uint32_t)kLdsTopNodes);
}
// LDS of a workgroup of the quad-walk frame kernels (dynamic, sized per launch): one 1 KiB row per stack entry the tree needs, the shared words, then
// the node copy — as many of the tree's first nodes as `budget` bytes leave room for, never fewer than the kLdsTopNodes (or the whole tree) that
// the shared row itself would hold. `bytes` is rounded up to the hardware's allocation granule.
struct WalkLdsPlan { uint32_t stack_rows, top_nodes, bytes; };
static constexpr uint32_t kLdsGranule = 512u;                   // LDS is allocated in 128-dword granules (the kernel descriptor's granulated size field)
static constexpr uint32_t kLdsPerCu = 160u * 1024u;
static constexpr uint32_t kLdsTracedBudget = kLdsPerCu / 4u;    // four workgroups per CU and nothing beside them: the traced kernels' registers allow no more traced waves
static constexpr uint32_t kLdsSharedBudget = kLdsPerCu / 5u;    // four traced workgroups leave 32 KiB of a CU for one workgroup of a light kernel (G-buffer, T-merge, post)
// The bytes a traced workgroup may use: `want` (kLdsSharedBudget unless a renderer is told otherwise: FRT_LDS_BUDGET) where the tree's stack rows
// and the shared words leave room in it for the kLdsTopNodes nodes every walk expects in LDS, kLdsTracedBudget otherwise.
inline uint32_t traced_lds_budget(uint32_t wg_rows, uint32_t want = kLdsSharedBudget) {
    const uint32_t least = (wg_rows < 2u ? 1u : wg_rows - 1u) * 1024u + kLdsSharedWords * 4u + (uint32_t)kLdsTopNodes * 128u;
    return want >= least ? want : std::max(want, kLdsTracedBudget);
}
#ifndef FRT_LDS_TOP_MAX
#define FRT_LDS_TOP_MAX 0xFFFFFFFFu      // (A/B builds only: a cap on the cached nodes)
#endif
// The G-buffer kernel's registers allow six and more waves per SIMD: its budget is the smallest share of a CU's LDS (a sixth, a fifth, a quarter,
// in whole granules) that holds the stack rows and the shared row. Every tree the builder accepts (31 stack rows at the most) gets a sixth or a
// fifth: at most kLdsSharedBudget, what four traced workgroups under that budget leave free on a CU.
inline uint32_t gbuffer_lds_budget(uint32_t wg_rows) {
    const uint32_t least = (wg_rows < 2u ? 2u : wg_rows) * 1024u;
    for (uint32_t wgs = 6u; wgs > 4u; --wgs) { const uint32_t b = kLdsPerCu / wgs / kLdsGranule * kLdsGranule; if (b >= least) return b; }
    return kLdsTracedBudget;
}
inline WalkLdsPlan walk_lds_plan(uint32_t wg_rows, uint32_t num_nodes4, uint32_t budget) {
    WalkLdsPlan p;
    p.stack_rows = wg_rows < 2u ? 1u : wg_rows - 1u;      // (wg_rows = stack need + 1; a one-node tree still gets a row to point at)
    const uint32_t fixed = p.stack_rows * 1024u + kLdsSharedWords * 4u;
    const uint32_t room = budget > fixed ? (budget - fixed) / 128u : 0u;
    p.top_nodes = std::min(std::min(num_nodes4, (uint32_t)FRT_LDS_TOP_MAX), std::max(room, (uint32_t)kLdsTopNodes));
    p.bytes = (std::max(fixed + p.top_nodes * 128u, (p.stack_rows + 1u) * 1024u) + kLdsGranule - 1u) / kLdsGranule * kLdsGranule;
    return p;
}

// continue_kernel: which parked paths workgroup `wg` of `threads` lanes resumes. Consecutive workgroups take consecutive regions (nsub: a power of
// two), so the workgroups that have paths are the first of the grid whatever the regions hold; lane t resumes slot region * rcap + offset + t of the
// queue while offset + t is below the region's fill. A grid of cont_grid_blocks workgroups visits every slot of every region exactly once.
struct RegionSlots { uint32_t region, offset; };
FRT_HD RegionSlots cont_region_slots(uint32_t wg, uint32_t nsub, uint32_t threads) {
    RegionSlots m;
    m.region = wg & (nsub - 1u);
    m.offset = (wg / nsub) * threads;
    return m;
}
inline uint32_t cont_grid_blocks(uint32_t capacity, uint32_t nsub, uint32_t threads) { return nsub * ((capacity / nsub + threads - 1u) / threads); }

// All launches are asynchronous on `stream` and cover rows [fv.y0, fv.y1).
hipError_t launch_gbuffer(const SceneView& sc, const FrameView& fv, hipStream_t stream, uint32_t wg_rows, uint32_t walk = kWalkQuad);      // wg_rows: TraceLaunch::wg_rows; walk: kWalkQuad or kWalkWide (primary rays are coherent: their nodes stay in HBM / L1)
hipError_t launch_trace_pixels(int stage, const SceneView& sc, const FrameView& fv, hipStream_t stream, const TraceLaunch& L);
bool trace_has_continuations(const TraceLaunch& L, uint32_t max_depth);
hipError_t launch_trace_continuations(int stage, const SceneView& sc, const FrameView& fv, hipStream_t stream, const TraceLaunch& L);
// LDS plan of the resident kernels for this scene: pair nodes cached (0 = the scene does not qualify), all triangle slots cached?
void resident_plan(const SceneView& sc, uint32_t& nodes, bool& tris);
// T-merge; `pending` (may be null): four ray counters {G closest, G any, T-trace closest, T-trace any} of a G-buffer + T-trace pair that
// ran ahead of its frame, added to `committed` and cleared.
// Both are region 0 of their counters; `nsub` regions of kRayRegionStride words each are committed.
hipError_t launch_merge(const SceneView& sc, const FrameView& fv, hipStream_t stream, unsigned long long* pending, unsigned long long* committed, uint32_t nsub);
hipError_t launch_post(const FrameView& fv, hipStream_t stream);
// Opt-in workgroup-compacting kernels (FRT_FLAG_COMPACTION): stage 1 = the FUSED temporal stage (trace + merge), stage 2 = spatial.
hipError_t launch_compact(int stage, const SceneView& sc, const FrameView& fv, hipStream_t stream);
}
