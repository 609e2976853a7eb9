// frt_renderer_state.hpp — private to the translation units of the renderer's C ABI (frt_renderer.hip: create, destroy and the frame loop;
// frt_scene_edit.hip: everything that edits the scene replica between frames; frt_scene_read.hip: everything that only reads it; frt_multi.hip;
// frt_scene_abi.cpp): the error and device helpers, the layout of the per-pixel buffers, the renderer's state structs and the few functions more than
// one of those files calls.
#pragma once
#include "frt_rebuild.hpp"      // (with frt_deform.hpp: frt_refit.hpp)
#include "frt_deform.hpp"
#include "frt_pose_batch.hpp"   // (frt_skin.hpp, frt_morph.hpp)
#include "frt_refit_device.hpp"
#include "frt_instance_edit.hpp"
#include "frt_material_edit.hpp"
#include "frt_mesh_edit.hpp"
#include "frt_scene_remove.hpp"
#include "frt_query.hpp"        // (frt_scene.hpp, frt_kernels.hpp)
#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdio>
#include <cstdlib>

#ifndef FRT_EXPERIMENTS
#define FRT_EXPERIMENTS 0      // 1: lib/libfrt_exp.so (`make experiments`): the measured-and-not-kept kernel designs and their FRT_* environment knobs
#endif

using namespace frt;

// The message frt_last_error returns is thread-local and lives in frt_scene_abi.cpp.
namespace frt { int set_error(int code, const std::string& msg); }
static inline int fail(int code, const std::string& msg) { return frt::set_error(code, msg); }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(FRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Every entry point that touches the device makes the renderer's device current and gives the caller's back on return (a host that
// drives several devices from one thread — frt_multi_renderer does — must not find its current device changed by a call).
struct DeviceGuard {
    int prev = -1; bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define FRT_DEVICE(r) DeviceGuard guard_((r)->device); if (!guard_.ok) return fail(FRT_ERR_HIP, "hipSetDevice failed")

// G-buffer, motion and candidate targets exist kGSets = kSpecDepth + 1 times. With one frame running ahead (the default) that is the
// reference's two ping-pong slots (gbuffer.rs:299): G-buffer(f+1) overwrites the set of frame f-1, whose last readers are done by then.
// Two frames ahead (kSpecDepth = 2, a third set: +60 B per pixel) was built and measured: 2.204 vs 2.208 ms — the ahead stream is in
// order, so frame f+2 cannot start before f+1's latency-bound tail has drained — and is therefore not compiled in. Which physical set
// holds which of the reference's two logical slots is tracked per frame (GSlots below), so any kSpecDepth works.
static const int kSpecDepth = 1;             // frames whose G-buffer + T-trace may run ahead
static const int kGSets = 3;                 // physical G-buffer sets addressable; a renderer owns `gsets` of them (2, strips under the pipeline 3)
enum { B_GPOS0 = 0, B_GNRM0 = B_GPOS0 + kGSets, B_GALB0 = B_GNRM0 + kGSets, B_GMOT0 = B_GALB0 + kGSets, B_CAND0 = B_GMOT0 + kGSets,
       B_RES0 = B_CAND0 + kGSets, B_RES1, B_RAW, B_DISP, B_ACC0, B_ACC1, B_COUNT };
// Buffers outside the arena (frt_renderer_arena_bytes stays 228 B per pixel): the third G-buffer set. Only strip renderers under the pipeline
// allocate them (frt_renderer::extras): with a third set the next frame's G-buffer + T-trace need not wait for this frame's T-merge.
static bool is_extra(int b) { return b < B_RES0 && (b % kGSets) == 2; }
static uint32_t bpp_of(int b) {
    if (b < B_GALB0) return 16u;        // gpos, gnormal
    if (b < B_GMOT0) return 4u;         // galbedo
    if (b < B_CAND0) return 8u;         // gmotion
    if (b < B_RES0) return 16u;         // candidate
    if (b <= B_RES1) return 32u;
    if (b == B_RAW) return 8u;
    if (b == B_DISP) return 4u;
    return 16u;                         // accumulation
}
struct GSlots { uint32_t g, gprev, aux; };   // physical sets: this frame's G-buffer, the previous logical slot's, and motion / candidate (= g under the pipeline)

// Device counters (unsigned long long each; one block of kRayRegionStride per region, summed by frt_renderer_stats): [0..7] committed rays per stage {closest, any}; [8] halo overflow;
// [9..12] PENDING rays of a G-buffer + T-trace pair that ran ahead of its frame (committed by its T-merge, dropped with a discarded speculation)
static const int kPending = 2;               // pending ray-count sets / T-trace events: consecutive speculated frames alternate (with three G-buffer sets
                                             // T-trace(f+1) may start before T-merge(f) has committed the counts of T-trace(f))
enum { C_STAGE = 0, C_HALO = 8, C_PENDING = 9, C_COUNT = 9 + 4 * kPending };   // a pending set of four per speculated frame in flight

#if FRT_EXPERIMENTS
// Everything the measured-and-not-kept kernel designs (csrc/experiments/frt_experiment_kernels.hpp) need in a renderer: their state, their FRT_*
// environment knobs, their allocations. Compiled into lib/libfrt_exp.so only (`make experiments`); the product library has none of it.
struct ExpState {
    int spec_depth = kSpecDepth;           // frames speculated ahead (FRT_SPEC_DEPTH, 0 .. kSpecDepth)
    long cont_grid = -1;                   // FRT_CONT_GRID: slots the spatial continuation grids cover at least (-1: half the stage's pixels)
    uint32_t* d_tiles = nullptr;           // per traced stage kTileStateWords words of sweep-direction state (FRT_TILE_ORDER=1), or null
    bool wavefront = false;                // ray-level wavefront (FRT_WAVEFRONT=1): per bounce depth a trace launch and a shade launch
    uint32_t* d_wf_words[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; uint32_t* d_wf_items[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint32_t* d_wf_hits[2] = {nullptr, nullptr}; uint32_t* d_wf_counts = nullptr;   // per stage: records x 2, item lists x 2, hit buffer; 2 x 96 counters
    bool stream_mode = false; uint32_t shade_min = 32, stream_slice = 8;   // stream kernel (resumable traversal) instead of continuation launches
    bool refill = false; uint32_t refill_min = 16;   // bounce kernel with lane refill (single cut) instead of continuation launches
    bool resident = false;                 // traced stages through the resident kernels (BVH cached in LDS, persistent workgroups)
    uint32_t res_nodes = 0; bool res_tris = false; uint32_t num_cus = 0, res_batch = 0;
    uint32_t* d_work = nullptr;            // work counters of the resident launches: [stage 1|2][launch slot][2]
};
#endif

// The state of the scene edits (frt_scene_edit.hip) is made of three things: Staging blocks for what a call uploads, OwnedBuf for the
// device buffers a call writes beside the replica, and one capacity record (PoolState) for every buffer of the replica that is sized by a count.

// What a call that edits or queries the scene replica stages its data through: one pinned host block and one device block, each grown on demand and
// never shrunk, and the event behind the last copy out of the pinned block.
struct Staging {
    uint8_t* h = nullptr; size_t h_cap = 0;
    uint8_t* d = nullptr; size_t d_cap = 0;
    hipEvent_t ev = nullptr; bool pending = false;
    // Both blocks hold at least this many bytes afterwards and the pinned one is free to be written: waits for `ev` if a copy out of it is pending.
    // The device block is replaced only after a wait for `stream`, whose kernels of an earlier call may still read it.
    int reserve(size_t h_bytes, size_t d_bytes, hipStream_t stream);
    int mark(hipStream_t stream);          // the copies out of the pinned block are enqueued: record `ev` (created here, at the first call)
    int upload(const void* src, size_t bytes, hipStream_t stream);      // reserve, `src` -> pinned block -> device block on `stream`, mark
    void release();
};

// A device buffer the renderer owns beside the scene replica: what a call builds into, and what then trades places with a buffer of the replica. It is
// allocated among the replica's allocations (frt_renderer::scene_allocs), so whichever side of a trade it ends on it is freed with the replica.
struct OwnedBuf {
    void* p = nullptr; size_t bytes = 0;
    // Room for `need` bytes: nothing when it is large enough; otherwise a wait for the main stream (a kernel of an earlier call may still use the
    // buffer), then it is freed and allocated anew (its contents are not kept).
    int ensure(frt_renderer* r, size_t need);
    // This buffer enters the replica as `live`; the one that leaves (with room for `live_bytes`) is what the next call builds into.
    template <class T> void trade(const T*& live, size_t live_bytes) { void* was = const_cast<T*>(live); live = static_cast<const T*>(p); p = was; bytes = live_bytes; }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void release(frt_renderer* r);         // behind a wait for the main stream: the buffer is freed (nothing if there is none)
};

// What frt_renderer_set_instance_transforms needs beside the scene replica, made at create. Device: the object-space positions of every
// mesh (16 B per vertex), the slot of every flattened triangle (4 B per triangle), one word for the scene extent and the moved-instance records
// (208 B each, staged through `rec`). Host: per instance what its record needs, the registered lights' emission, the level ranges of both trees.
// What frt_renderer_set_instance_transforms_ex adds for FRT_TRANSFORM_DEVICE ("Transforms from device memory"; frt_refit_device.hpp), made
// at the first such call, each with room for the instance capacity. `consts` restates the host's per-instance bookkeeping: an edit that changes what it
// holds only clears consts_ok, and the next device call uploads it again (through `up`). `m` holds every instance's matrix and is the truth from the
// first device call on: RefitState::inst[].m (with .w2o and .flip) is then a mirror that may be stale, and a call that reads it reads `m` back first.
// mirror_stale implies m_ok; m_ok is cleared only while the mirror is current (then the next device call uploads the mirror).
struct DeviceTransformState {
    OwnedBuf consts, m, last;              // [InstanceConst], [4 float4], [uint32_t] per instance
    Staging up;                            // the pinned block the two tables are uploaded through
    bool consts_ok = false, m_ok = false, mirror_stale = false;
    uint32_t* d_reject = nullptr;          // [0] the flag of the call in flight, [1] the calls rejected so far (TransformInput::reject)
};

struct RefitState {
    bool ok = false;                      // level ranges found (both trees are numbered breadth-first: frt_bvh.cpp)
    const float4* d_pos = nullptr;
    const uint32_t* d_slot_of = nullptr;
    const unsigned int* d_ext = nullptr;
    std::vector<uint32_t> pos_offset;      // per mesh: its first vertex in d_pos
    std::vector<InstanceRec> inst;         // mesh, first_tri, tri_count, light link
    std::vector<frt_light> lights;         // the scene's lights as uploaded (emission of the registered ones)
    std::vector<uint32_t> index_offset;    // per mesh
    std::vector<uint32_t> pair_levels, quad_levels;   // level L of a tree = nodes [levels[L], levels[L + 1])
    Staging rec;                           // the moved-instance records of one call (MovedInstance)
    // frt_renderer_set_mesh_vertices ("Deforming meshes"): per mesh its vertex count and first attribute; `def`: the staging of one call of the family
    // that deforms, its sections named by frt_scene_edit.hip's DeformLayout (vertices) or PoseBatchLayout (every posing call).
    std::vector<uint32_t> vert_count, attr_offset;
    std::vector<uint32_t> mesh_tris;       // per mesh: its triangles (what an added instance of it brings)
    Staging def;
    // FRT_DEFORM_RECOMPUTE_NORMALS: per mesh its vertex -> corner adjacency on the device, [offsets: vert_count + 1 | corners: 3 mesh_tris] (null: not made
    // yet; ensure_adjacency makes it at the mesh's first such call). Mesh-local numbers: a pool that moves or grows leaves it valid, remove_meshes renumbers it.
    std::vector<const uint32_t*> adj;
    // FRT_DEFORM_DEVICE: [0] the flag of the call in flight, [1] the calls rejected so far (frt_deform.hpp: DeformInput); made at the first such call.
    uint32_t* d_reject = nullptr;
    // What a bind call leaves with a mesh: one device buffer and how many joints or targets it was bound with (0: nothing bound). The lists may be
    // shorter than the mesh list; remove_meshes frees a leaving mesh's bindings and renumbers the rest.
    // `mode`: of a skin, how it is posed (0 the linear blend, FRT_SKIN_DUAL_QUATERNION); it travels with the binding wherever that goes.
    struct MeshBinding { OwnedBuf buf; uint32_t count = 0, mode = 0; };
    // frt_renderer_set_mesh_skin / _set_mesh_pose ("Skinning"): a skin is [bind positions 16 nverts | weights 16 nverts | joints 8 nverts], `count` its
    // joints. `skin_up`: the pinned block a bind call's weights and joints go through. `skinned`: the posed positions of the posing call in flight, a single
    // mesh's or a batch's ("Posing several meshes"), [the summed vertex counts] float4, whatever launch wrote them last.
    std::vector<MeshBinding> skins;
    Staging skin_up;
    OwnedBuf skinned;
    // frt_renderer_set_mesh_morph_targets / _set_mesh_morph_weights / _set_mesh_pose_ex ("Morph targets"): targets are [base positions 16 nverts |
    // deltas, target-major, 12 nverts per target], `count` the targets. `morph_up`: the pinned block a bind call's deltas go through (a block of its
    // own: a morph bind does not wait for a skin bind's copies). A call without a palette morphs into `skinned`; with one it morphs into `morphed`, as
    // large as `skinned`, which the skin launch then reads as its bind pose.
    std::vector<MeshBinding> morphs;
    Staging morph_up;
    OwnedBuf morphed;
    DeviceTransformState xf;               // FRT_TRANSFORM_DEVICE
#if FRT_EXPERIMENTS
    OwnedBuf tri_normals;                 // lib/libfrt_exp.so, FRT_NORMALS_TRI_PASS=1: the scratch of the triangle pass (NormalArgs::tri_scratch)
#endif
    uint32_t color_layers = 0, data_layers = 0;   // texture layers of the replica (the material and texture edits check against them)
};

// What frt_renderer_rebuild_tree adds ("Rebuild"), allocated at the first call: the scratch of the kernels, the triangle slots and the
// id -> slot table that are NOT in use (they trade places with the replica's at every successful rebuild) and up to two quad-node buffers of
// rebuild_max_nodes() nodes, built into in turn (the host-built tree's buffer may be smaller than a device tree needs, so it is never built into;
// the second one is allocated by the second rebuild). Each has room for a tree over the triangle capacity.
struct RebuildState {
    RebuildScratch scratch;
    OwnedBuf tris, slot_of;
    OwnedBuf nodes[2];
    bool done = false;                     // the replica's quad tree is a device rebuild: the pair tree and its quantised form are stale
    uint32_t origin = 0;                   // frt_renderer_tree_stats: 1 the Morton tree, 2 the refined tree
    uint32_t last[4] = {0, 0, 0, 0};       // frt_renderer_rebuild_stats
};

// What frt_renderer_add_instances / _remove_instances add, allocated at the first call, each with room for the triangle or instance
// capacity: an edit writes them, and its rebuild reads them.
struct InstanceEditState {
    OwnedBuf tris, slot_of;                // never part of the replica: the rebuild makes the replica's next slots and table out of them
    OwnedBuf shade_tris, instances;        // they trade places with the replica's when the edit's rebuild succeeds
    Staging rec;                           // the records of one call (AppendInstance / RemovedRange)
};

// The one capacity record. Every buffer of the replica that is sized by a count belongs to one of these pools; pool_count() tells how many elements of a
// pool are in use, cap[] how many its buffers have room for. A renderer's pools are as uploaded, exactly as large as their counts (cap 0), until a
// call gives one a capacity apart from its count: a growth (frt_renderer_add_*, _register_*_light: DESIGN.md §14, §15) or, before a count goes down, a
// removal (§14, §16). A capacity at least doubles when it grows (the texture arrays, 4 MiB a layer: by max(4, count / 2) layers), is never shrunk, and
// a growth is a new allocation plus a device-to-device copy behind a wait for the stream. A renderer that never makes such a call allocates nothing.
enum { kPoolVerts = 0, kPoolIndices, kPoolMeshes, kPoolMaterials, kPoolLights, kPoolColor, kPoolData,      // §15, §16
       kPoolTris, kPoolInstances,                                                                           // §14
       kPoolCount };
struct PoolState {
    uint32_t cap[kPoolCount] = {};         // 0: the pool is as uploaded, exactly as large as its count
    uint32_t growths = 0;                  // calls that had to grow a pool of §15 (frt_renderer_pool_counts)
    // The decoded normal of every vertex (xyz, 0), indexed as SceneView::attributes: a buffer of the vertex pool that is not part of the SceneView, made
    // at the first call that needs it (ensure_normals); set_mesh_vertices keeps it up, add_instances reads it.
    const float4* d_normals = nullptr;
    Staging up;                            // what one call of §15 uploads: the pinned block and, for add_meshes, the device block its kernel reads
};

// What frt_renderer_remove_materials / _meshes / _lights / _texture add, allocated at the first such call. A pool that closes up is
// compacted out of place into its `spare`, which then trades places with the replica's buffer: what left the replica is what the next removal from that
// pool writes, behind every kernel that read it (the same stream). A spare has room for its pool's capacity.
enum { kSparePos = 0, kSpareAttrs, kSpareNormals, kSpareIndices, kSpareMeshInfos, kSpareMaterials, kSpareLights, kSpareCount };
struct RemoveState {
    OwnedBuf spare[kSpareCount];
    Staging tab;                           // the tables of one call: old -> new ids and removed spans
};

// What frt_renderer_bind_rig leaves with the renderer ("Animation"; frt_animation.hip): the rig's block on the device, the palette
// [4 njoints] float4 and the weights [ntargets] its kernel writes, and the meshes frt_renderer_animate poses. A binding's number is its index; an unbound
// one stays in the list, empty (live == false).
// frt_renderer_bind_rig_instances ("Node animation") leaves a binding of kind kRigInstances in the same list: the rig's block, `ids` [n] the bound
// instances, `tab` = [the nodes' stored indices, n words padded to 16 bytes | root, 16 floats | offsets, 16 n floats] (root and offsets only when
// given) and `mats` [4 n] float4, what its kernel writes and the device transform reads. `instance_ids` is the host's copy of `ids`, which
// remove_instances renumbers; ids_stale: the device copy is uploaded again by the next animate_instances.
// frt_renderer_set_rig_masks ("Layering clips") leaves either kind `masks` = [nmasks][nnodes] floats in the block's node order, allocated once for
// FRT_MAX_RIG_MASKS masks so that a later set is a copy in stream order and nothing else; `place` (the caller's node index -> the block's) and `nnodes`
// are the rig's, kept from bind time.
// frt_renderer_set_rig_goals / _set_rig_goal_targets ("Inverse kinematics") leave either kind `goals` = [FRT_MAX_RIG_GOALS frt_rig_goal with stored node
// indices | enter [nnodes] | exit [nnodes]] and `goal_targets` = [FRT_MAX_RIG_GOALS frt_rig_goal_target], allocated at the first set with a goal and
// freed with the binding; `enter` / `exit` (the pre-order numbers of the stored nodes, from bind time) and `goal_defs` (the host's copy of the definitions: what host targets are
// checked against) stay on the host.
enum { kRigMeshes = 0, kRigInstances = 1 };
struct RigBinding {
    OwnedBuf rig, palette, weights;
    uint32_t njoints = 0, ntargets = 0, nclips = 0;
    std::vector<uint32_t> mesh_ids;
    bool live = false;
    uint32_t kind = kRigMeshes;
    OwnedBuf ids, tab, mats;
    std::vector<uint32_t> instance_ids;
    bool has_root = false, has_offsets = false, ids_stale = false;
    OwnedBuf masks;
    uint32_t nmasks = 0, nnodes = 0;
    std::vector<uint32_t> place;
    OwnedBuf goals, goal_targets;
    uint32_t ngoals = 0;
    std::vector<uint32_t> enter, exit;
    std::vector<frt_rig_goal> goal_defs;
    void release(frt_renderer* r) { for (OwnedBuf* b : {&rig, &palette, &weights, &ids, &tab, &mats, &masks, &goals, &goal_targets}) b->release(r); }
};
// What frt_renderer_animate_cast adds ("Animating a cast"): one device buffer, grown on demand and never shrunk, that holds what the halves of a call
// read as ONE range each — [ids of every instance entry | their matrices | the palettes of every mesh entry | their weights] — beside the bindings' own
// buffers, which the kernel writes too. The entry table goes through frt_renderer::rig_up, its device block included.
struct CastState { OwnedBuf buf; };
// One mesh of a cast's mesh half and what it is posed under (device memory: a slice of CastState::buf), and the whole call as frt_scene_edit.hip's
// apply_cast takes it: the instance half's records, the mesh half's meshes and the one range of palette columns and of weights the pose batch tests.
struct CastMesh { uint32_t mesh; const float* palette; uint32_t njoints; const float* weights; uint32_t ntargets; };
struct CastApply {
    uint32_t ninst = 0; const uint32_t* ids = nullptr; const float* mats = nullptr;
    std::vector<CastMesh> meshes;
    const float* palettes = nullptr; uint32_t cols = 0;
    const float* weights = nullptr; uint32_t nweights = 0;
    bool recompute = false;
};

struct frt_renderer {
    int device = 0;
    hipStream_t stream = nullptr;          // the chain: T-merge -> spatial pixels -> spatial continuations (and everything, without FRT_FLAG_PIPELINE)
    bool own_stream = false;
    hipStream_t ahead = nullptr;           // FRT_FLAG_PIPELINE: G-buffer(f+1), T-trace(f+1)
    hipStream_t edge = nullptr;            // FRT_FLAG_PIPELINE, strips: the spatial pixel launches of the halo-dependent edge rows (beside the interior launch)
    hipStream_t edge2 = nullptr;           // ... the second edge of a middle strip: its launch runs beside the first one's instead of behind it
    hipEvent_t ev_spix = nullptr, ev_tt[kPending] = {}, ev_tail = nullptr, ev_tm[2] = {nullptr, nullptr}, ev_edge = nullptr, ev_edge2 = nullptr, ev_edge_ready = nullptr;
    bool tail_pending = false;             // work enqueued on `ahead` that the main stream has not been ordered behind yet
    bool edge_in_flight = false, edge2_in_flight = false;
    uint32_t W = 0, H = 0, max_depth = 8, rb = 0, re = 0, flags = 0, motion_halo = 0;
    uint32_t frame_count = 0;
    float jitter[2] = {0.0f, 0.0f};        // PostParams.jitter of the next post stage
    SceneView sv{};
    std::vector<void*> scene_allocs;
    uint8_t* arena = nullptr;
    bool own_arena = false;
    size_t arena_bytes = 0;
    size_t off[B_COUNT] = {};
    unsigned long long* d_counters = nullptr;
    // continuation queues: per traced stage one word buffer per path segment parity (the second only with two cuts or more)
    uint32_t* d_qwords[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint32_t qcap = 0, qcap_max = 0;       // slots per queue; upper bound = every traced pixel parks
    uint32_t qslots[2][2] = {{0, 0}, {0, 0}};   // slots of each word buffer [stage][first | second buffer], derived from qcap (alloc_queues)
    uint64_t qbytes = 0;                   // device bytes of the word buffers
    bool qcap_fixed = false;               // capacity given by the caller: never grown
    uint32_t nsub = 16;                    // regions of every continuation queue and of the ray counters (frt_mono.hpp: ContQueue; chosen by the sweep of profiles/r12_experiments/regional_queues.md)
    uint32_t* d_qcount = nullptr;          // [stage 1|2][launch parity 0|1] sets of nsub counter lines, then [stage] overflow blocks (frt_renderer.hip: qcount_set_words)
    uint32_t* h_qseen = nullptr; uint32_t* d_qseen = nullptr;   // one word of mapped host memory: set by a wave that found its queue full (ContQueue::seen)
    uint32_t qparity[2] = {0, 0};
    uint32_t ncuts = 2, cuts[kMaxCuts] = {3, 4, 0, 0};   // measured best on the Cornell Box
    bool vote = false;                     // traced kernels with the voting BVH walk (set from the size of the scene's quad tree, upload_scene)
    uint32_t walk = kWalkQuad, wide_lds_bytes = 0, wg_rows = 0;      // which tree the traced kernels walk and how (frt_kernels.hpp: kWalk*; upload_scene)
    uint32_t lds_budget = 0;               // bytes of LDS a traced workgroup may use; 0 = the default (frt_kernels.hpp: traced_lds_budget; FRT_LDS_BUDGET)
#if FRT_EXPERIMENTS
    ExpState x;                            // lib/libfrt_exp.so only: state and FRT_* knobs of the measured-and-not-kept kernel designs (csrc/experiments/)
#endif
    frt_stats stats{};
    struct Timed { hipEvent_t a, b; int slot; };
    std::vector<Timed> pending;
    std::vector<hipEvent_t> event_pool;
    // frame in progress
    bool failed = false;                   // a HIP call failed in the middle of a frame: the stage flags and stream order are no longer trustworthy; render calls
                                           // return FRT_ERR_STATE until frt_renderer_clear
    bool frame_open = false, g_done = false, tt_done = false, tm_done = false, s_started = false, s_inner_done = false, s_edge_done = false;
    bool from_speculation = false;
    Timed s_timer{};
    bool s_timed = false;
    // which physical G set holds the reference's logical slot 0 / 1 (frame_count % 2) for the NEXT G-buffer launch, the sets of the frame in
    // progress and of the last finished frames (what reads through the ABI see)
    uint32_t logical_phys[2] = {0, 1};
    GSlots cur_slots{0, 1, 0}, last_slots{0, 1, 0}, before_last_slots{1, 0, 0};
    uint32_t last_parity = 0;              // frame_count % 2 of the frame that recorded last_slots (the counter may move without a frame: end_frame, reset)
    // speculation: G-buffer + T-trace of the next frames, enqueued on `ahead` under the cameras a static scene will present
    struct Spec { frt_camera_uniform cam; uint32_t frame; GSlots slots; uint32_t logical_before[2]; int idx; };
    std::vector<Spec> specs;               // oldest first, at most kSpecDepth
    int spec_next_idx = 0, cur_spec_idx = 0;
    bool camera_static = false;
    frt_camera_uniform last_cam{}, cur_cam{};
    bool have_last_cam = false;
    uint8_t* extras = nullptr; size_t extras_bytes = 0;      // the buffers of is_extra(), when this renderer has them
    uint32_t gsets = 2;                    // G-buffer sets in use
    uint64_t serial = 0;                   // frames finished since creation (never reset: parity of the per-frame events)
    RefitState rf;
    RebuildState rbt;
    InstanceEditState ie;
    PoolState pools;
    RemoveState rm;
    // The host-pointer ray queries: both blocks [input | output] of a call. Such a call is synchronous — the last call's copies are done
    // when the next one starts — so this one is never marked: no event is created, recorded or waited for.
    Staging qry;
    // The material, light and texture edits: the pinned block of one call and, for frt_renderer_set_instance_materials, its records on the device.
    Staging look;
    std::vector<RigBinding> rigs;          // frt_renderer_bind_rig
    Staging rig_up;                        // the pinned block a rig is uploaded through
    CastState cast;                        // frt_renderer_animate_cast
    void* buf(int b) const { return is_extra(b) ? extras + off[b] : arena + off[b]; }
    bool pipeline() const { return ahead != nullptr; }
};

template <class T, class D>
static int upload(frt_renderer* r, const std::vector<T>& v, const D** out) {
    void* d = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_TRY(hipMalloc(&d, bytes));
    r->scene_allocs.push_back(d);
    if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const D*>(d);
    return FRT_OK;
}

#ifndef FRT_VOTE_MIN_NODES
#define FRT_VOTE_MIN_NODES 32768      // (4 MiB of quad nodes; A/B builds: 0 = every scene votes, a huge value = none does)
#endif
static const size_t kVoteMinQuadNodes = FRT_VOTE_MIN_NODES;
// The walk of a tree of `quad_nodes` nodes: the voting loop from kVoteMinQuadNodes on. FRT_WALK_VOTE=0|1 in the environment overrides the size rule
// (tests run both walks over one small scene; tools time both over one scene).
static inline bool walk_votes(size_t quad_nodes) {
    if (const char* e = getenv("FRT_WALK_VOTE")) return atoi(e) != 0;
    return quad_nodes >= kVoteMinQuadNodes;
}

namespace frt {
int fence_ahead(frt_renderer* r);                                  // frt_renderer.hip
int sync_all(frt_renderer* r);
int drop_speculation(frt_renderer* r);
int upload_refit_data(frt_renderer* r, const SceneBuilder& b);    // frt_scene_edit.hip
// What a call `what` refuses before it looks at its own arguments, in this order: a null handle, then the `parts` it asks for.
enum { kNotFailed = 1, kBetweenFrames = 2, kRefit = 4, kQuadTree = 8, kEditChecks = kNotFailed | kBetweenFrames | kQuadTree,
       kLookChecks = kNotFailed | kBetweenFrames };      // (the edits of §13, §15 and §16 involve no tree: every renderer takes them)
int check_entry(const frt_renderer* r, const std::string& what, unsigned parts);
uint32_t pool_count(const frt_renderer* r, int pool);             // elements of a pool (PoolState) in use
int ensure_normals(frt_renderer* r);                              // PoolState::d_normals exists afterwards
int check_device_block(const frt_renderer* r, const void* p, size_t bytes, size_t align, const char* call, const char* what, const char* flag);      // frt_scene_edit.hip: its check_device_input, for the other files
int apply_cast(frt_renderer* r, const CastApply& c);              // frt_scene_edit.hip: the two halves of frt_renderer_animate_cast in one call frame
// "" when the batch (check_pose_batch) and then every mesh of it, as its single call checks it ("mesh N: ..."), can be posed: with `skin` under a palette of
// `njoints` joints, with `morph` under `ntargets` weights. host_memory: the entries of the palette and of the weights, the same for every mesh, are read
// (at the first mesh only); otherwise the two pointers are only compared with null. What set_mesh_poses, bind_rig, animate and animate_cast share.
std::string check_posed_meshes(const frt_renderer* r, uint32_t n, const uint32_t* mesh_ids, bool skin, const void* palette, uint32_t njoints, bool morph, const void* weights, uint32_t ntargets, bool host_memory);
}
