// frt_animation.hip — the device form of an animated rig (include/frt.h: frt_renderer_bind_rig, _animate, _read_rig_pose, _unbind_rig; DESIGN.md §11,
// "Animation"; _bind_rig_instances, _animate_instances: "Node animation"; _animate_cast: "Animating a cast"). Built with the library's contract flags. No arithmetic is written here: the kernel calls the FRT_HD functions of frt_animation.hpp that
// frt_rig_evaluate calls on the host, so the palette and the weights have the host's bits. The _blend forms of the three animate calls ("Blending
// clips") run the same kernels with their list of samples; frt_rig_evaluate_blend is their host form. The _layers forms ("Layering clips") run the
// same kernel texts instantiated for a list of layers; frt_rig_evaluate_layers is their host form.
//
// The kernel is ONE workgroup of four waves per rig. (1) Every lane builds the local matrix of a node (sampling the clip's channels of that node),
// strided by the workgroup's size, into LDS. (2) The globals are propagated level by level: a node's parent lies on the level above, which is complete
// behind the workgroup barrier that ends it; a node reads its parent's global and its own local and writes its own global in place, so no two lanes touch
// one entry. The level bounds are the same words for every lane: every barrier is reached by the whole workgroup. (3) One lane per joint multiplies the
// joint node's global with the inverse bind matrix and stores four float4 (16-byte vector stores); one lane per target samples a morph weight.
// LDS: FRT_MAX_RIG_NODES x 64 B = 64 KiB, column c of node n at [c * FRT_MAX_RIG_NODES + n], so the lanes of a wave, on consecutive nodes, read and
// write consecutive 16-byte words.
#include "frt_renderer_state.hpp"
#include "frt_animation.hpp"

namespace frt {

static const int kRigBlock = 256;      // four waves of 64
static const uint32_t kRigLds = FRT_MAX_RIG_NODES;

__device__ inline m4 rig_lds_load(const float4* g, uint32_t n) {
    m4 m;
#pragma unroll
    for (int c = 0; c < 4; ++c) { const float4 q = g[(uint32_t)c * kRigLds + n]; m.c[c] = mk4(q.x, q.y, q.z, q.w); }
    return m;
}
__device__ inline void rig_lds_store(float4* g, uint32_t n, const m4& m) {
#pragma unroll
    for (int c = 0; c < 4; ++c) g[(uint32_t)c * kRigLds + n] = make_float4(m.c[c].x, m.c[c].y, m.c[c].z, m.c[c].w);
}

// What the host calls have refused of a sample list: uniform, asked in front of the first barrier.
__device__ inline bool rig_samples_ok(const RigHeader& h, const frt_clip_sample* s, uint32_t ns) {
    if (ns == 0u || ns > FRT_MAX_BLEND_SAMPLES) return false;
    bool positive = false;
    for (uint32_t i = 0; i < ns; ++i) {
        if (s[i].clip >= h.nclips) return false;
        positive = positive || s[i].weight > 0.0f;
    }
    return positive;
}
// ... and of a layer list ("Layering clips"): check_clip_layers restated on the layer words, which are uniform, a mask index the binding's masks do not
// have included (rig_local_matrix_layers reads no mask at or beyond nmasks, and with this guard no kernel runs with a layer that names one).
__device__ inline bool rig_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool rig_layers_ok(const RigHeader& h, const frt_clip_layer* l, uint32_t nl, uint32_t nmasks, const float* masks) {
    if (nl == 0u || nl > FRT_MAX_LAYERS || nmasks > FRT_MAX_RIG_MASKS || (nmasks && !masks)) return false;
    for (uint32_t i = 0; i < nl; ++i) {
        if (l[i].mode > (uint32_t)FRT_LAYER_ADDITIVE || (l[i].flags & ~FRT_LAYER_KEEP_MORPH) || l[i].clip >= h.nclips) return false;
        if (l[i].mode == (uint32_t)FRT_LAYER_ADDITIVE) { if (l[i].ref_clip >= h.nclips) return false; }
        else if (l[i].ref_clip != 0u || !(l[i].ref_time == 0.0f)) return false;
        if (!rig_finite(l[i].time) || !rig_finite(l[i].ref_time) || !rig_finite(l[i].weight) || l[i].weight < 0.0f) return false;
        if (l[i].mode == (uint32_t)FRT_LAYER_OVERRIDE && l[i].weight > 1.0f) return false;
        if (l[i].mask != FRT_LAYER_NO_MASK && l[i].mask >= nmasks) return false;
    }
    return l[0].mode == (uint32_t)FRT_LAYER_BLEND && l[0].mask == FRT_LAYER_NO_MASK && l[0].weight > 0.0f && l[0].flags == 0u;
}

// The POSE SOURCE of a kernel: what phase (1) folds into a node's local matrix and what a morph weight is taken from. Either a list of samples
// ("Blending clips"; the single-clip calls pass a list of one sample of weight 1, which the contract makes the single clip's bits) or a list of
// layers with the binding's masks ("Layering clips"). The kernels below are templates over it, so the single-clip and blend calls run instantiations
// that hold no layer code at all, and the layered calls instantiations of their own. A source's words are the same for every lane (a kernel
// argument, or read through the block's index: scalar loads), so every branch on a count, a mode or a flag is taken by the whole workgroup. The one
// divergent branch of the layers, e > 0 under a mask, lies inside phase (1), where there is no barrier; the mask read is masks[mask * N + n],
// consecutive lanes on consecutive nodes.
struct RigSamples {
    const frt_clip_sample* s; uint32_t n;
    __device__ bool ok(const RigHeader& h) const { return rig_samples_ok(h, s, n); }
    __device__ m4 local(RigView v, uint32_t node) const { return rig_local_matrix_blend(v, n, s, node); }
    __device__ float morph(RigView v, uint32_t c) const { return rig_morph_weight_blend(v, n, s, c); }
};
struct RigLayers {
    const frt_clip_layer* l; uint32_t n, nmasks; const float* masks;
    __device__ bool ok(const RigHeader& h) const { return rig_layers_ok(h, l, n, nmasks, masks); }
    __device__ m4 local(RigView v, uint32_t node) const { return rig_local_matrix_layers(v, n, l, nmasks, masks, node); }
    __device__ float morph(RigView v, uint32_t c) const { return rig_morph_weight_layers(v, n, l, c); }
};
// The lists the one-rig kernels take by value as a kernel argument; a cast's entries point at theirs.
struct RigSampleList {
    uint32_t n, pad0, pad1, pad2; frt_clip_sample s[FRT_MAX_BLEND_SAMPLES];
    __device__ RigSamples source() const { return RigSamples{s, n}; }
};
static_assert(sizeof(frt_clip_sample) == 16 && sizeof(RigSampleList) == 16 + 16 * FRT_MAX_BLEND_SAMPLES, "RigSampleList layout");
struct RigLayerList {
    uint32_t n, nmasks; const float* masks; frt_clip_layer l[FRT_MAX_LAYERS];      // masks: the binding's, [nmasks][nnodes] in the block's node order
    __device__ RigLayers source() const { return RigLayers{l, n, nmasks, masks}; }
};
static_assert(sizeof(frt_clip_layer) == 32 && sizeof(RigLayerList) == 16 + 32 * FRT_MAX_LAYERS, "RigLayerList layout");

// Phases (1) and (2) of every kernel: the global matrix of every node < N is in `g` behind the last barrier. Called by the whole workgroup with uniform
// arguments (the source and the level bounds are the same words for every lane). Phase (1) is one lane, one node: every sample's or layer's clip
// sampled into translation, rotation and scale, folded in registers as one running pose (rig_local_matrix_blend, rig_local_matrix_layers), the local
// matrix stored.
template <class Source>
__device__ inline void rig_globals_to_lds(RigView v, const RigHeader& h, const Source& src, float4* g, uint32_t N) {
    const uint32_t* words = v.w;
    const uint32_t tid = threadIdx.x;
    for (uint32_t n = tid; n < N; n += (uint32_t)kRigBlock) rig_lds_store(g, n, src.local(v, n));
    __syncthreads();
    for (uint32_t level = 1u; level < h.nlevels; ++level) {
        const uint32_t begin = words[h.level_begin + level], end = words[h.level_begin + level + 1u];
        for (uint32_t n = begin + tid; n < end && n < N; n += (uint32_t)kRigBlock) {
            const uint32_t p = words[h.parent + n];
            if (p < n) rig_lds_store(g, n, mul(rig_lds_load(g, p), rig_lds_load(g, n)));
        }
        __syncthreads();
    }
}

// The GOALS of a kernel ("Inverse kinematics"), its second policy: none (the single-clip and blend calls, and a layered call on a binding without
// goals: instantiations that hold no goal code at all), or the binding's. Bound goals are device memory the binding owns: `g` [n] the definitions
// with stored node indices, `enter` / `exit` [nnodes] the pre-order numbers behind them in the same buffer, `t` [FRT_MAX_RIG_GOALS] the targets.
struct RigNoGoals {
    static constexpr bool any = false;
    __device__ bool ok(uint32_t) const { return true; }
};
// The third policy ("Chain IK") is the second with Chain = true: launched only when the binding (for a cast: any entry's binding) carries a
// FRT_GOAL_CHAIN goal, so bindings with two-bone and aim goals only run the instantiations without a line of chain code.
template <bool Chain>
struct RigBoundGoalsT {
    static constexpr bool any = true;
    static constexpr bool chain = Chain;
    uint32_t n, pad; const frt_rig_goal* g; const uint32_t* enter; const uint32_t* exit; const frt_rig_goal_target* t;
    // What set_rig_goals has refused, restated on the goal words (uniform): the count, the kinds, nodes < N; of a chain (whose mid is its sweeps
    // and whose reserved word is K, the bones of its path) the two caps. Asked in front of the first barrier.
    __device__ bool ok(uint32_t N) const {
        if (n > FRT_MAX_RIG_GOALS) return false;
        if (n && (!g || !enter || !exit || !t)) return false;
        for (uint32_t i = 0; i < n; ++i) {
            if constexpr (Chain) {
                if (g[i].kind == FRT_GOAL_CHAIN) {
                    if (g[i].root >= N || g[i].tip >= N || g[i].mid < 1u || g[i].mid > FRT_IK_CHAIN_MAX_SWEEPS || g[i].reserved < 1u || g[i].reserved >= FRT_IK_CHAIN_MAX_NODES) return false;
                    continue;
                }
            }
            if (g[i].kind > (uint32_t)FRT_GOAL_AIM || g[i].root >= N || g[i].mid >= N || g[i].tip >= N) return false;
        }
        return true;
    }
};
typedef RigBoundGoalsT<false> RigBoundGoals;
typedef RigBoundGoalsT<true> RigChainGoals;
static_assert(sizeof(frt_rig_goal) == 32 && sizeof(frt_rig_goal_target) == 32 && sizeof(RigBoundGoals) == 40 && sizeof(RigChainGoals) == 40, "goal layouts");

// "Chain IK": one FRT_GOAL_CHAIN goal, the chain held in registers across the lanes of a wave. The solve is strictly sequential (every step reads
// the tip the step before it moved), so it is not run as READ / BARRIER / WRITE rounds (2 S K workgroup barriers and S K sweeps over the N nodes)
// but inside each wave, with no barrier and no LDS traffic:
// GATHER: each of the four waves holds the whole chain, redundantly (every lane computes the same, nobody is elected). Lane j <= K of a wave owns
// c_j, P_j and D_j; the lanes find their node by the uniform parent walk from the tip, K steps over the rig block's parents, and read their
// node's origin from LDS once. Lanes above K own the tip: what they compute is never read.
// SOLVE: S K steps; P_K and P_k come by wave broadcast (__shfl from a uniform lane), every lane computes the same R through ik_chain_step, and
// the lanes with j > k (j >= k for D) update their own words under a lane predicate. No register array is indexed by a variable.
// APPLY: one barrier (every wave has read its origins before a global is rewritten), then all 256 lanes stride over the N nodes in whole rounds,
// so that every lane of a wave executes every __shfl: the chain's enter / exit numbers are broadcast lane by lane, the deepest hit is kept and
// clamped to K - 1, the sixteen words of D_j come from lane j of the node's own wave (__shfl with a per-lane source; all sixteen, so that
// mul(D_j, G) has the host's operands to the bit whatever D's last row holds), and mul(D_j, G) is stored in place. One barrier follows. Both
// barriers are reached by the whole workgroup whether or not the goal is on. Called with uniform arguments.
__device__ inline float rig_lane(float x, uint32_t lane) { return __shfl(x, (int)lane); }
__device__ inline uint32_t rig_lane(uint32_t x, uint32_t lane) { return (uint32_t)__shfl((int)x, (int)lane); }
__device__ inline f3 rig_lane(f3 p, uint32_t lane) { return mk3(rig_lane(p.x, lane), rig_lane(p.y, lane), rig_lane(p.z, lane)); }
__device__ inline f4 rig_lane(f4 p, uint32_t lane) { return mk4(rig_lane(p.x, lane), rig_lane(p.y, lane), rig_lane(p.z, lane), rig_lane(p.w, lane)); }
__device__ inline void rig_apply_chain(const frt_rig_goal& gl, const frt_rig_goal_target& t, const uint32_t* enter, const uint32_t* exit, const uint32_t* parent, float4* g, uint32_t N) {
    const uint32_t K = gl.reserved, S = gl.mid;      // (ok() has held them to 1 .. 31 and 1 .. 16, root and tip below N)
    const uint32_t lane = threadIdx.x & 63u;
    const bool on = ik_target_ok(t);                 // (uniform)
    uint32_t mine = gl.tip, en = 0u, ex = 0u;
    m4 D = ik_identity();
    if (on) {
        uint32_t c = gl.tip;
        for (uint32_t i = K; i > 0u; --i) {          // c: c_i
            if (lane == i) mine = c;
            const uint32_t p = parent[c];
            c = p < c ? p : c;                       // (a root has no parent: set_rig_goals has counted the path, so none is met)
        }
        if (lane == 0u) mine = c;
        en = enter[mine]; ex = exit[mine];
        const float4 o = g[3u * kRigLds + mine];
        f3 P = mk3(o.x, o.y, o.z);
        const f3 Te = ik_chain_target(rig_lane(P, K), t);
#pragma unroll 1
        for (uint32_t s = 0; s < S; ++s) {
#pragma unroll 1
            for (uint32_t k = K; k-- > 0u;) {
                m4 R;
                if (!ik_chain_step(rig_lane(P, k), rig_lane(P, K), Te, R)) continue;      // (the same for every lane)
                if (lane > k) P = ik_point(R, P);
                if (lane >= k) D = mul(R, D);
            }
        }
    }
    __syncthreads();
    if (on) {
        for (uint32_t base = 0; base < N; base += (uint32_t)kRigBlock) {
            const uint32_t n = base + threadIdx.x;
            const bool live = n < N;
            const uint32_t at = enter[live ? n : 0u];
            bool hit = false;
            uint32_t j = 0u;
            for (uint32_t i = 0; i <= K; ++i) {      // nested subtrees: the last hit is the deepest
                const uint32_t a = rig_lane(en, i), b = rig_lane(ex, i);
                if (a <= at && at < b) { hit = true; j = i; }
            }
            j = j < K ? j : K - 1u;
            m4 Dj;
#pragma unroll
            for (int c = 0; c < 4; ++c) Dj.c[c] = rig_lane(D.c[c], j);
            if (live && hit) rig_lds_store(g, n, mul(Dj, rig_lds_load(g, n)));
        }
    }
    __syncthreads();
}
// Between phases (2) and (3): every goal is one round. READ: every lane reads the goal's words (global memory) and its pivots' globals (LDS) — the
// same addresses for every lane — and computes the same matrices; no lane is elected and nothing is shared. BARRIER (every lane has read the pivots
// before one of them is written). WRITE: the lanes stride over all N nodes, test membership by enter / exit and store mul(D, G) in place, one lane
// per entry. BARRIER. Both barriers are reached by the whole workgroup in every round: a skipped goal skips its stores only. Called with uniform
// arguments behind the last barrier of rig_globals_to_lds.
template <class Goals>
__device__ inline void rig_apply_goals(const Goals& goals, RigView v, const RigHeader& h, float4* g, uint32_t N) {
    if constexpr (Goals::any) {
#pragma unroll 1
        for (uint32_t i = 0; i < goals.n; ++i) {
            const frt_rig_goal gl = goals.g[i];
            if constexpr (Goals::chain) {      // ("Chain IK": a uniform branch; a chain goal is one round of its own, with the two barriers of every round)
                if (gl.kind == FRT_GOAL_CHAIN) { rig_apply_chain(gl, goals.t[i], goals.enter, goals.exit, v.w + h.parent, g, N); continue; }
            }
            const IkDelta d = ik_goal_delta(gl, goals.t[i], rig_lds_load(g, gl.root), rig_lds_load(g, gl.mid), rig_lds_load(g, gl.tip));
            __syncthreads();
            if (d.on) {
                for (uint32_t n = threadIdx.x; n < N; n += (uint32_t)kRigBlock) {
                    m4 G = rig_lds_load(g, n);
                    if (ik_move_node(d, goals.enter, goals.exit, n, G)) rig_lds_store(g, n, G);
                }
            }
            __syncthreads();
        }
    }
}

template <class List, class Goals>
__global__ void __launch_bounds__(kRigBlock) rig_evaluate_kernel(const uint32_t* words, const List list, const Goals goals, float4* palette, float* weights) {
    __shared__ float4 g[4u * kRigLds];
    RigView v; v.w = words;
    const RigHeader h = v.h();
    const uint32_t tid = threadIdx.x;
    const uint32_t N = h.nnodes < kRigLds ? h.nnodes : kRigLds;      // (bind_rig refuses a larger rig)
    const auto src = list.source();
    if (!src.ok(h) || !goals.ok(N)) return;                          // (animate refuses it; uniform: no barrier is skipped by a part of the workgroup)
    if (h.njoints) {
        rig_globals_to_lds(v, h, src, g, N);
        rig_apply_goals(goals, v, h, g, N);
        for (uint32_t j = tid; j < h.njoints; j += (uint32_t)kRigBlock) {
            const uint32_t n = words[h.joint_node + j];
            if (n >= N) continue;
            const m4 m = mul(rig_lds_load(g, n), load_m4(v.f(h.inv_bind) + (size_t)16u * j));
#pragma unroll
            for (int c = 0; c < 4; ++c) palette[4u * j + (uint32_t)c] = make_float4(m.c[c].x, m.c[c].y, m.c[c].z, m.c[c].w);
        }
    }
    for (uint32_t c = tid; c < h.ntargets; c += (uint32_t)kRigBlock) weights[c] = src.morph(v, c);
}

// frt_renderer_animate_instances ("Node animation"): phases (1) and (2) as above, whether or not the rig has joints; (3) one lane per bound instance,
// strided by the workgroup's size, loads its node's global from LDS, applies root and offset through rig_node_matrix (the host's text) and stores four
// float4 into the binding's matrices. `nodes` [n]: stored node indices; `root` [16] and `offsets` [16 n]: null when the binding has none.
template <class List, class Goals>
__global__ void __launch_bounds__(kRigBlock) rig_nodes_kernel(const uint32_t* words, const List list, const Goals goals, uint32_t n, const uint32_t* nodes, const float* root, const float* offsets, float4* mats) {
    __shared__ float4 g[4u * kRigLds];
    RigView v; v.w = words;
    const RigHeader h = v.h();
    const uint32_t N = h.nnodes < kRigLds ? h.nnodes : kRigLds;      // (bind_rig_instances refuses a larger rig)
    const auto src = list.source();
    if (!src.ok(h) || !goals.ok(N)) return;                          // (animate_instances refuses it; uniform, in front of the first barrier)
    rig_globals_to_lds(v, h, src, g, N);
    rig_apply_goals(goals, v, h, g, N);
    for (uint32_t k = threadIdx.x; k < n; k += (uint32_t)kRigBlock) {
        const uint32_t node = nodes[k];
        if (node >= N) continue;                                     // (bind_rig_instances has checked it)
        const m4 m = rig_node_matrix(rig_lds_load(g, node), root, offsets ? offsets + (size_t)16u * k : nullptr);
#pragma unroll
        for (int c = 0; c < 4; ++c) mats[4u * k + (uint32_t)c] = make_float4(m.c[c].x, m.c[c].y, m.c[c].z, m.c[c].w);
    }
}

// frt_renderer_animate_cast ("Animating a cast"): the two kernels above as one, ONE WORKGROUP PER ENTRY of the call's table (gridDim.x = entries), so a
// cast of any size is one launch and its rigs are walked side by side on as many CUs. An entry is 112 bytes, 16-byte aligned, and is read through the
// block's index alone: its words are the same for every lane (scalar loads), so every branch on them is taken by the whole workgroup, and all of them
// sit in front of the first barrier or behind the last. Phases (1) and (2) are rig_globals_to_lds; phase (3) is that of the entry's kind, with every
// store made twice: into the binding's own buffer (what read_rig_pose / read_rig_instances return) and into the entry's slice of the call's buffer,
// where the instance half finds all ids and matrices, and the mesh half all palettes and weights, as one range each. 64 KiB of static LDS: two
// workgroups per CU.
struct CastEntry {
    const uint32_t* words;      // the binding's rig block
    const frt_clip_sample* samples;      // the entry's samples [nsamples], behind the table in the same device block
    uint32_t nsamples;
    uint32_t kind, n;           // kRigMeshes | kRigInstances; instances: the bound instances
    uint32_t pad0;
    float4* own; float4* all;   // meshes: the palette [4 njoints]; instances: the matrices [4 n] — the binding's, and the slice of the call's buffer
    float* own_w; float* all_w; // meshes: the weights [ntargets]
    const uint32_t* nodes; const float* root; const float* offsets;      // instances: as rig_nodes_kernel takes them
    const uint32_t* ids; uint32_t* all_ids;                              // instances: the binding's ids [n] and their slice of the call's ids
    uint64_t pad1;
    typedef frt_clip_sample Item;
    void set_list(const Item* items, uint32_t count, const RigBinding&) { samples = items; nsamples = count; }
    __device__ RigSamples source() const { return RigSamples{samples, nsamples}; }
};
static_assert(sizeof(CastEntry) == 112 && sizeof(CastEntry) % 16 == 0, "CastEntry layout");
// The entry of a layered cast ("Layering clips"): CastEntry with the entry's layers in place of its samples, and its own binding's masks.
struct CastLayersEntry {
    const uint32_t* words;
    const frt_clip_layer* layers;      // the entry's layers [nlayers], behind the table in the same device block
    uint32_t nlayers;
    uint32_t kind, n;
    uint16_t nmasks, ngoals;           // the binding's masks [nmasks][nnodes], in the block's node order, and its goals ("Inverse kinematics"): both at most 16
    float4* own; float4* all;
    float* own_w; float* all_w;
    const uint32_t* nodes; const float* root; const float* offsets;
    const uint32_t* ids; uint32_t* all_ids;
    const float* masks;
    const uint8_t* goals;              // "Inverse kinematics": the binding's goal buffer [FRT_MAX_RIG_GOALS goals | enter | exit] and its targets
    const frt_rig_goal_target* goal_targets;
    typedef frt_clip_layer Item;
    void set_list(const Item* items, uint32_t count, const RigBinding& b) {
        layers = items; nlayers = count; nmasks = (uint16_t)b.nmasks; masks = b.nmasks ? b.masks.as<const float>() : nullptr;
        ngoals = (uint16_t)b.ngoals; goals = b.ngoals ? b.goals.as<const uint8_t>() : nullptr; goal_targets = b.ngoals ? b.goal_targets.as<const frt_rig_goal_target>() : nullptr;
    }
    __device__ RigLayers source() const { return RigLayers{layers, nlayers, nmasks, masks}; }
};
static_assert(sizeof(CastLayersEntry) == 128 && sizeof(CastLayersEntry) % 16 == 0 && alignof(CastLayersEntry) <= 16, "CastLayersEntry layout");
// The goals of a cast's entry: the entry's own binding's (an entry without goals runs the loop zero times); none for a cast without goals.
template <bool Chain>
__device__ inline RigBoundGoalsT<Chain> rig_goals_at(const uint8_t* buf, const frt_rig_goal_target* t, uint32_t n, uint32_t nnodes) {
    const uint32_t* tree = reinterpret_cast<const uint32_t*>(buf + sizeof(frt_rig_goal) * FRT_MAX_RIG_GOALS);
    return RigBoundGoalsT<Chain>{n, 0u, reinterpret_cast<const frt_rig_goal*>(buf), tree, tree + nnodes, t};
}
template <class Goals, class Entry> struct CastGoals { __device__ static RigNoGoals of(const Entry&, uint32_t) { return RigNoGoals(); } };
template <bool Chain> struct CastGoals<RigBoundGoalsT<Chain>, CastLayersEntry> {
    __device__ static RigBoundGoalsT<Chain> of(const CastLayersEntry& e, uint32_t nnodes) { return e.ngoals ? rig_goals_at<Chain>(e.goals, e.goal_targets, e.ngoals, nnodes) : RigBoundGoalsT<Chain>{0u, 0u, nullptr, nullptr, nullptr, nullptr}; }
};

__device__ inline void rig_store_twice(float4* own, float4* all, uint32_t k, const m4& m) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 q = make_float4(m.c[c].x, m.c[c].y, m.c[c].z, m.c[c].w);
        own[4u * k + (uint32_t)c] = q;
        all[4u * k + (uint32_t)c] = q;
    }
}
template <class Entry, class Goals>
__global__ void __launch_bounds__(kRigBlock) rig_cast_kernel(const Entry* table) {
    __shared__ float4 g[4u * kRigLds];
    const Entry e = table[blockIdx.x];
    RigView v; v.w = e.words;
    const RigHeader h = v.h();
    const uint32_t tid = threadIdx.x;
    const uint32_t N = h.nnodes < kRigLds ? h.nnodes : kRigLds;      // (the bind calls refuse a larger rig)
    const auto src = e.source();
    const Goals goals = CastGoals<Goals, Entry>::of(e, h.nnodes);      // (enter and exit lie behind the definitions, nnodes words each)
    if (!src.ok(h) || !goals.ok(N)) return;                          // (animate_cast refuses it; uniform, in front of the first barrier)
    const bool instances = e.kind == (uint32_t)kRigInstances;
    if (instances || h.njoints) { rig_globals_to_lds(v, h, src, g, N); rig_apply_goals(goals, v, h, g, N); }
    if (instances) {
        for (uint32_t k = tid; k < e.n; k += (uint32_t)kRigBlock) {
            e.all_ids[k] = e.ids[k];
            const uint32_t node = e.nodes[k];
            if (node >= N) {      // (bind_rig_instances has checked it) the call's slice holds what the binding holds
#pragma unroll
                for (int c = 0; c < 4; ++c) e.all[4u * k + (uint32_t)c] = e.own[4u * k + (uint32_t)c];
                continue;
            }
            rig_store_twice(e.own, e.all, k, rig_node_matrix(rig_lds_load(g, node), e.root, e.offsets ? e.offsets + (size_t)16u * k : nullptr));
        }
        return;
    }
    for (uint32_t j = tid; j < h.njoints; j += (uint32_t)kRigBlock) {
        const uint32_t n = e.words[h.joint_node + j];
        if (n >= N) {
#pragma unroll
            for (int c = 0; c < 4; ++c) e.all[4u * j + (uint32_t)c] = e.own[4u * j + (uint32_t)c];
            continue;
        }
        rig_store_twice(e.own, e.all, j, mul(rig_lds_load(g, n), load_m4(v.f(h.inv_bind) + (size_t)16u * j)));
    }
    for (uint32_t c = tid; c < h.ntargets; c += (uint32_t)kRigBlock) {
        const float w = src.morph(v, c);
        e.own_w[c] = w;
        e.all_w[c] = w;
    }
}

} // namespace frt

static RigBinding* find_binding(frt_renderer* r, uint32_t binding) { return binding < r->rigs.size() && r->rigs[binding].live ? &r->rigs[binding] : nullptr; }
// The binding gets the first free number: an unbound one is used again.
static uint32_t keep_binding(frt_renderer* r, const RigBinding& b) {
    size_t slot = 0;
    while (slot < r->rigs.size() && r->rigs[slot].live) ++slot;
    if (slot == r->rigs.size()) r->rigs.push_back(b); else r->rigs[slot] = b;
    return (uint32_t)slot;
}
static bool finite_bits(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
// The list a kernel takes: the n samples a call has checked, or the single clip of a call without a blend as one sample of weight 1.
static RigSampleList sample_list(uint32_t n, const frt_clip_sample* s) {
    RigSampleList l;
    memset(&l, 0, sizeof(l));
    l.n = n;
    memcpy(l.s, s, (size_t)n * sizeof(frt_clip_sample));
    return l;
}
static RigSampleList one_clip(uint32_t clip, float time) { const frt_clip_sample s{clip, time, 1.0f, 0u}; return sample_list(1u, &s); }
// ... and the n layers a call has checked against the binding's mask count, with the binding's masks ("Layering clips").
static RigLayerList layer_list(uint32_t n, const frt_clip_layer* l, const RigBinding& b) {
    RigLayerList list;
    memset(&list, 0, sizeof(list));
    list.n = n; list.nmasks = b.nmasks; list.masks = b.nmasks ? b.masks.as<const float>() : nullptr;
    memcpy(list.l, l, (size_t)n * sizeof(frt_clip_layer));
    return list;
}

// frt_renderer_animate_instances, _animate_instances_blend and _animate_instances_layers behind their checks: the kernel, then the device transform.
// The goals a layered call on binding b launches with ("Inverse kinematics"): for a binding that carries some.
template <bool Chain = false>
static RigBoundGoalsT<Chain> bound_goals(const RigBinding& b) {
    const uint32_t* tree = reinterpret_cast<const uint32_t*>(b.goals.as<const uint8_t>() + sizeof(frt_rig_goal) * FRT_MAX_RIG_GOALS);
    return RigBoundGoalsT<Chain>{b.ngoals, 0u, b.goals.as<const frt_rig_goal>(), tree, tree + b.nnodes, b.goal_targets.as<const frt_rig_goal_target>()};
}
// "Chain IK": whether the binding's goals hold a chain, which is what picks the third goal policy.
static bool has_chain_goal(const RigBinding& b) {
    for (uint32_t i = 0; i < b.ngoals; ++i) if (b.goal_defs[i].kind == FRT_GOAL_CHAIN) return true;
    return false;
}

template <class List, class Goals = RigNoGoals>
static int move_bound_instances(frt_renderer* r, const std::string& call, RigBinding* b, const List& list, const Goals& goals = Goals()) {
    const uint32_t n = (uint32_t)b->instance_ids.size();
    {
        // The kernel writes the binding's matrices only, which nothing but the device transform of an earlier animate_instances reads: on this stream, in front of it.
        FRT_DEVICE(r);
        if (b->ids_stale) {      // (remove_instances has renumbered the instances)
            if (const int rc = r->rig_up.reserve((size_t)n * 4, 0, r->stream)) return rc;
            memcpy(r->rig_up.h, b->instance_ids.data(), (size_t)n * 4);
            HIP_TRY(hipMemcpyAsync(b->ids.p, r->rig_up.h, (size_t)n * 4, hipMemcpyHostToDevice, r->stream));
            if (const int rc = r->rig_up.mark(r->stream)) return rc;
            b->ids_stale = false;
        }
        const uint8_t* tab = b->tab.as<const uint8_t>();
        const size_t node_bytes = ((size_t)n * 4 + 15u) & ~(size_t)15u;
        const float* root = b->has_root ? reinterpret_cast<const float*>(tab + node_bytes) : nullptr;
        const float* offsets = b->has_offsets ? reinterpret_cast<const float*>(tab + node_bytes + (b->has_root ? 64u : 0u)) : nullptr;
        hipLaunchKernelGGL((rig_nodes_kernel<List, Goals>), dim3(1), dim3(kRigBlock), 0, r->stream, b->rig.as<const uint32_t>(), list, goals, n, reinterpret_cast<const uint32_t*>(tab), root, offsets, b->mats.as<float4>());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { r->failed = true; return fail(FRT_ERR_HIP, call + ": " + hipGetErrorString(e)); }
    }
    return frt_renderer_set_instance_transforms_ex(r, n, b->ids.as<const uint32_t>(), b->mats.as<const float>(), FRT_TRANSFORM_DEVICE);
}
// frt_renderer_animate, _animate_blend and _animate_layers behind their checks of the list: the meshes as animate checks them, the kernel, then the
// pose batch.
template <class List, class Goals = RigNoGoals>
static int pose_bound_meshes(frt_renderer* r, const std::string& call, RigBinding* b, const List& list, uint32_t flags, const Goals& goals = Goals()) {
    const uint32_t n = (uint32_t)b->mesh_ids.size();
    const std::string bad = check_posed_meshes(r, n, b->mesh_ids.data(), b->njoints != 0, b->palette.p, b->njoints, b->ntargets != 0, b->weights.p, b->ntargets, false);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, call + ": " + bad);
    {
        // The kernel writes the binding's palette and weights only, which nothing but the pose launches of an earlier animate read: on this stream, in front of it.
        FRT_DEVICE(r);
        hipLaunchKernelGGL((rig_evaluate_kernel<List, Goals>), dim3(1), dim3(kRigBlock), 0, r->stream, b->rig.as<const uint32_t>(), list, goals, b->palette.as<float4>(), b->weights.as<float>());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { r->failed = true; return fail(FRT_ERR_HIP, call + ": " + hipGetErrorString(e)); }
    }
    return frt_renderer_set_mesh_poses(r, n, b->mesh_ids.data(), b->njoints ? b->palette.as<float>() : nullptr, b->njoints,
                                       b->ntargets ? b->weights.as<float>() : nullptr, b->ntargets, flags | FRT_DEFORM_DEVICE);
}

// What check_cast_entries asks about the renderer's bindings.
static std::vector<CastBinding> cast_bindings(const frt_renderer* r) {
    std::vector<CastBinding> info(r->rigs.size());
    for (size_t i = 0; i < r->rigs.size(); ++i) {
        const RigBinding& b = r->rigs[i];
        const std::vector<uint32_t>& ids = b.kind == kRigInstances ? b.instance_ids : b.mesh_ids;
        info[i].live = b.live; info[i].kind = b.kind; info[i].nclips = b.nclips; info[i].njoints = b.njoints; info[i].ntargets = b.ntargets;
        info[i].ids = ids.data(); info[i].n = (uint32_t)ids.size();
    }
    return info;
}
// frt_renderer_animate_cast, _animate_cast_blend and _animate_cast_layers behind the checks of their entries (`entries`: the bindings, as cast_layout
// takes them; `ranges`: every entry's samples among samples [nsamples] — for the layered cast, with Entry = CastLayersEntry, its layers among the
// layers): every mesh entry's meshes as animate checks them, the layout of the call's buffer, ONE staged copy — the entry table, the samples and the
// ids of the instance bindings remove_instances has renumbered — ONE launch, then frt_scene_edit.hip's apply_cast.
// Past the first call of a steady cast nothing here allocates, waits for the stream or copies synchronously: the pinned block's event has long passed
// when the next call comes.
struct CastRange { uint32_t first, count; };
template <class Entry, class Goals = RigNoGoals>
static int run_cast(frt_renderer* r, const std::string& call_name, uint32_t n, const frt_cast_entry* entries, const CastRange* ranges,
                    const std::vector<CastBinding>& info, uint32_t nsamples, const typename Entry::Item* samples, uint32_t flags) {
    std::string bad;
    for (uint32_t k = 0; k < n && bad.empty(); ++k) {
        const RigBinding& b = r->rigs[entries[k].binding];
        if (b.kind != kRigMeshes) continue;
        bad = check_posed_meshes(r, (uint32_t)b.mesh_ids.size(), b.mesh_ids.data(), b.njoints != 0, b.palette.p, b.njoints, b.ntargets != 0, b.weights.p, b.ntargets, false);
        if (!bad.empty()) bad = "entry " + std::to_string(k) + ": " + bad;
    }
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, call_name + ": " + bad);
    const CastLayout l = cast_layout(n, entries, info.data());
    CastApply call;
    call.recompute = (flags & FRT_DEFORM_RECOMPUTE_NORMALS) != 0;
    {
        // The kernel writes the bindings' own buffers and the call's buffer only, which nothing but the launches of an earlier call read: on this stream, in front of it.
        FRT_DEVICE(r);
        if (const int rc = r->cast.buf.ensure(r, l.bytes)) return rc;
        uint8_t* all = r->cast.buf.as<uint8_t>();
        const size_t table_bytes = (size_t)n * sizeof(Entry), sample_bytes = (size_t)nsamples * sizeof(typename Entry::Item);      // (both multiples of 16)
        size_t stale_bytes = 0;
        for (uint32_t k = 0; k < n; ++k) { const RigBinding& b = r->rigs[entries[k].binding]; if (b.kind == kRigInstances && b.ids_stale) stale_bytes += b.instance_ids.size() * 4; }
        if (const int rc = r->rig_up.reserve(table_bytes + sample_bytes + stale_bytes, table_bytes + sample_bytes, r->stream)) return rc;
        Entry* table = reinterpret_cast<Entry*>(r->rig_up.h);
        memcpy(r->rig_up.h + table_bytes, samples, sample_bytes);
        const typename Entry::Item* dev_samples = reinterpret_cast<const typename Entry::Item*>(r->rig_up.d + table_bytes);
        size_t stale_at = table_bytes + sample_bytes;
        for (uint32_t k = 0; k < n; ++k) {
            RigBinding& b = r->rigs[entries[k].binding];
            Entry e;
            memset(&e, 0, sizeof(e));
            e.words = b.rig.as<const uint32_t>(); e.set_list(dev_samples + ranges[k].first, ranges[k].count, b); e.kind = b.kind;
            if (b.kind == kRigInstances) {
                const uint32_t ni = (uint32_t)b.instance_ids.size();
                if (b.ids_stale) {      // (remove_instances has renumbered the instances) in front of the launch, as animate_instances uploads them
                    memcpy(r->rig_up.h + stale_at, b.instance_ids.data(), (size_t)ni * 4);
                    HIP_TRY(hipMemcpyAsync(b.ids.p, r->rig_up.h + stale_at, (size_t)ni * 4, hipMemcpyHostToDevice, r->stream));
                    stale_at += (size_t)ni * 4;
                    b.ids_stale = false;
                }
                const uint8_t* tab = b.tab.as<const uint8_t>();
                const size_t node_bytes = ((size_t)ni * 4 + 15u) & ~(size_t)15u;
                e.n = ni; e.nodes = reinterpret_cast<const uint32_t*>(tab);
                e.root = b.has_root ? reinterpret_cast<const float*>(tab + node_bytes) : nullptr;
                e.offsets = b.has_offsets ? reinterpret_cast<const float*>(tab + node_bytes + (b.has_root ? 64u : 0u)) : nullptr;
                e.own = b.mats.as<float4>(); e.all = reinterpret_cast<float4*>(all + l.mats_off) + 4u * (size_t)l.first[k];
                e.ids = b.ids.as<const uint32_t>(); e.all_ids = reinterpret_cast<uint32_t*>(all + l.ids_off) + l.first[k];
            } else {
                e.own = b.palette.as<float4>(); e.all = reinterpret_cast<float4*>(all + l.pal_off) + l.first[k];
                e.own_w = b.weights.as<float>(); e.all_w = reinterpret_cast<float*>(all + l.wt_off) + l.first_weight[k];
                for (uint32_t m : b.mesh_ids)
                    call.meshes.push_back(CastMesh{m, b.njoints ? reinterpret_cast<const float*>(e.all) : nullptr, b.njoints, b.ntargets ? e.all_w : nullptr, b.ntargets});
            }
            table[k] = e;
        }
        HIP_TRY(hipMemcpyAsync(r->rig_up.d, r->rig_up.h, table_bytes + sample_bytes, hipMemcpyHostToDevice, r->stream));
        if (const int rc = r->rig_up.mark(r->stream)) return rc;
        hipLaunchKernelGGL((rig_cast_kernel<Entry, Goals>), dim3(n), dim3(kRigBlock), 0, r->stream, reinterpret_cast<const Entry*>(r->rig_up.d));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { r->failed = true; return fail(FRT_ERR_HIP, call_name + ": " + hipGetErrorString(e)); }
        call.ninst = l.ninst; call.ids = reinterpret_cast<const uint32_t*>(all + l.ids_off); call.mats = reinterpret_cast<const float*>(all + l.mats_off);
        if (l.cols) { call.palettes = reinterpret_cast<const float*>(all + l.pal_off); call.cols = l.cols; }
        if (l.nweights) { call.weights = reinterpret_cast<const float*>(all + l.wt_off); call.nweights = l.nweights; }
    }
    return apply_cast(r, call);
}

extern "C" {

int frt_renderer_bind_rig(frt_renderer* r, const frt_rig* rig, const uint32_t* mesh_ids, uint32_t n, uint32_t* binding_out) {
    if (const int rc = check_entry(r, "bind_rig", kEditChecks | kRefit)) return rc;
    if (!rig || !binding_out) return fail(FRT_ERR_INVALID_ARG, "bind_rig: null");
    const RigHeader h = rig->view().h();
    if (h.nnodes > FRT_MAX_RIG_NODES) return fail(FRT_ERR_INVALID_ARG, "bind_rig: " + std::to_string(h.nnodes) + " nodes, more than FRT_MAX_RIG_NODES");
    const std::string bad = check_posed_meshes(r, n, mesh_ids, h.njoints != 0, rig, h.njoints, h.ntargets != 0, rig, h.ntargets, false);      // (the pointers are only compared with null)
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "bind_rig: " + bad);
    FRT_DEVICE(r);
    RigBinding b;
    int rc;
    if ((rc = b.rig.ensure(r, rig->words.size() * 4))) return rc;
    if ((rc = b.palette.ensure(r, (size_t)h.njoints * 64))) { b.rig.release(r); return rc; }
    if ((rc = b.weights.ensure(r, (size_t)h.ntargets * 4))) { b.rig.release(r); b.palette.release(r); return rc; }
    rc = r->rig_up.reserve(rig->words.size() * 4, 0, r->stream);
    if (rc == FRT_OK) {
        memcpy(r->rig_up.h, rig->words.data(), rig->words.size() * 4);
        hipError_t e = hipMemcpyAsync(b.rig.p, r->rig_up.h, rig->words.size() * 4, hipMemcpyHostToDevice, r->stream);
        if (e == hipSuccess) e = hipMemsetAsync(b.palette.p, 0, b.palette.bytes, r->stream);
        if (e == hipSuccess) e = hipMemsetAsync(b.weights.p, 0, b.weights.bytes, r->stream);
        rc = e == hipSuccess ? r->rig_up.mark(r->stream) : fail(FRT_ERR_HIP, std::string("bind_rig: ") + hipGetErrorString(e));
    }
    if (rc) { b.rig.release(r); b.palette.release(r); b.weights.release(r); return rc; }
    b.njoints = h.njoints; b.ntargets = h.ntargets; b.nclips = h.nclips; b.mesh_ids.assign(mesh_ids, mesh_ids + n); b.live = true;
    b.nnodes = h.nnodes; b.place = rig->place; { RigTree t = rig_tree(rig->view()); b.enter.swap(t.enter); b.exit.swap(t.exit); }
    *binding_out = keep_binding(r, b);
    return FRT_OK;
}

int frt_renderer_bind_rig_instances(frt_renderer* r, const frt_rig* rig, uint32_t n, const uint32_t* instance_ids, const uint32_t* nodes, const float* root, const float* offsets, uint32_t* binding_out) {
    if (const int rc = check_entry(r, "bind_rig_instances", kEditChecks | kRefit)) return rc;
    if (!rig || !binding_out) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: null");
    const RigHeader h = rig->view().h();
    if (h.nnodes > FRT_MAX_RIG_NODES) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: " + std::to_string(h.nnodes) + " nodes, more than FRT_MAX_RIG_NODES");
    if (n == 0 || n > FRT_MAX_RIG_INSTANCES) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: " + std::to_string(n) + " instances (1 .. FRT_MAX_RIG_INSTANCES)");
    if (!instance_ids || !nodes) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: null ids or nodes");
    const size_t ninst = r->rf.inst.size();
    std::vector<uint8_t> seen(ninst, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t id = instance_ids[k];
        if (id >= ninst) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: instance id " + std::to_string(id) + " out of range (" + std::to_string(ninst) + " instances)");
        if (seen[id]) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: instance id " + std::to_string(id) + " given twice");
        seen[id] = 1;
        if (nodes[k] >= h.nnodes) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: node " + std::to_string(nodes[k]) + " is not a node (" + std::to_string(h.nnodes) + " nodes)");
    }
    for (size_t i = 0; root && i < 16; ++i) if (!finite_bits(root[i])) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: a root entry is not finite");
    for (size_t i = 0; offsets && i < (size_t)16 * n; ++i) if (!finite_bits(offsets[i])) return fail(FRT_ERR_INVALID_ARG, "bind_rig_instances: an offsets entry is not finite");
    FRT_DEVICE(r);
    // one pinned block: [rig | ids | tab], tab = [nodes, padded to 16 bytes | root | offsets]
    const size_t rig_bytes = rig->words.size() * 4, id_bytes = (size_t)n * 4, node_bytes = ((size_t)n * 4 + 15u) & ~(size_t)15u;
    const size_t root_bytes = root ? 64u : 0u, off_bytes = offsets ? (size_t)n * 64 : 0u, tab_bytes = node_bytes + root_bytes + off_bytes;
    RigBinding b;
    int rc;
    if ((rc = b.rig.ensure(r, rig_bytes)) == FRT_OK && (rc = b.ids.ensure(r, id_bytes)) == FRT_OK && (rc = b.tab.ensure(r, tab_bytes)) == FRT_OK) rc = b.mats.ensure(r, (size_t)n * 64);
    if (rc == FRT_OK) rc = r->rig_up.reserve(rig_bytes + id_bytes + tab_bytes, 0, r->stream);
    if (rc == FRT_OK) {
        uint8_t* up = r->rig_up.h;
        uint8_t* tab = up + rig_bytes + id_bytes;
        memcpy(up, rig->words.data(), rig_bytes);
        memcpy(up + rig_bytes, instance_ids, id_bytes);
        memset(tab, 0, node_bytes);
        for (uint32_t k = 0; k < n; ++k) { const uint32_t stored = rig->place[nodes[k]]; memcpy(tab + (size_t)4 * k, &stored, 4); }
        if (root) memcpy(tab + node_bytes, root, 64);
        if (offsets) memcpy(tab + node_bytes + root_bytes, offsets, off_bytes);
        hipError_t e = hipMemcpyAsync(b.rig.p, up, rig_bytes, hipMemcpyHostToDevice, r->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.ids.p, up + rig_bytes, id_bytes, hipMemcpyHostToDevice, r->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.tab.p, tab, tab_bytes, hipMemcpyHostToDevice, r->stream);
        if (e == hipSuccess) e = hipMemsetAsync(b.mats.p, 0, (size_t)n * 64, r->stream);
        rc = e == hipSuccess ? r->rig_up.mark(r->stream) : fail(FRT_ERR_HIP, std::string("bind_rig_instances: ") + hipGetErrorString(e));
    }
    if (rc) { b.release(r); return rc; }
    b.kind = kRigInstances; b.nclips = h.nclips; b.instance_ids.assign(instance_ids, instance_ids + n); b.has_root = root != nullptr; b.has_offsets = offsets != nullptr; b.live = true;
    b.nnodes = h.nnodes; b.place = rig->place; { RigTree t = rig_tree(rig->view()); b.enter.swap(t.enter); b.exit.swap(t.exit); }
    *binding_out = keep_binding(r, b);
    return FRT_OK;
}

int frt_renderer_animate_instances(frt_renderer* r, uint32_t binding, uint32_t clip, float time) {
    if (const int rc = check_entry(r, "animate_instances", kEditChecks | kRefit)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate_instances: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigInstances) return fail(FRT_ERR_INVALID_ARG, "animate_instances: binding " + std::to_string(binding) + " binds meshes (frt_renderer_animate)");
    if (clip >= b->nclips) return fail(FRT_ERR_INVALID_ARG, "animate_instances: clip " + std::to_string(clip) + " out of range (" + std::to_string(b->nclips) + " clips)");
    if (!finite_bits(time)) return fail(FRT_ERR_INVALID_ARG, "animate_instances: time is not finite");
    return move_bound_instances(r, "animate_instances", b, one_clip(clip, time));
}

int frt_renderer_animate_instances_blend(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_sample* samples) {
    if (const int rc = check_entry(r, "animate_instances_blend", kEditChecks | kRefit)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate_instances_blend: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigInstances) return fail(FRT_ERR_INVALID_ARG, "animate_instances_blend: binding " + std::to_string(binding) + " binds meshes (frt_renderer_animate_blend)");
    const std::string bad = check_blend_samples(n, samples, b->nclips);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_instances_blend: " + bad);
    return move_bound_instances(r, "animate_instances_blend", b, sample_list(n, samples));
}

int frt_renderer_read_rig_instances(frt_renderer* r, uint32_t binding, float* mats_out) {
    if (const int rc = check_entry(r, "read_rig_instances", kNotFailed)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b || b->kind != kRigInstances) return fail(FRT_ERR_INVALID_ARG, "read_rig_instances: unknown instance rig binding " + std::to_string(binding));
    if (!mats_out) return fail(FRT_ERR_INVALID_ARG, "read_rig_instances: null");
    FRT_DEVICE(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(mats_out, b->mats.p, b->instance_ids.size() * 64, hipMemcpyDeviceToHost));
    return FRT_OK;
}

int frt_renderer_animate(frt_renderer* r, uint32_t binding, uint32_t clip, float time, uint32_t flags) {
    if (const int rc = check_entry(r, "animate", kEditChecks | kRefit)) return rc;
    if (flags & ~FRT_DEFORM_RECOMPUTE_NORMALS) return fail(FRT_ERR_INVALID_ARG, "animate: unknown flag bits");
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigMeshes) return fail(FRT_ERR_INVALID_ARG, "animate: binding " + std::to_string(binding) + " binds instances (frt_renderer_animate_instances)");
    if (clip >= b->nclips) return fail(FRT_ERR_INVALID_ARG, "animate: clip " + std::to_string(clip) + " out of range (" + std::to_string(b->nclips) + " clips)");
    if ((__builtin_bit_cast(uint32_t, time) & 0x7f800000u) == 0x7f800000u) return fail(FRT_ERR_INVALID_ARG, "animate: time is not finite");
    return pose_bound_meshes(r, "animate", b, one_clip(clip, time), flags);
}

int frt_renderer_animate_blend(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_sample* samples, uint32_t flags) {
    if (const int rc = check_entry(r, "animate_blend", kEditChecks | kRefit)) return rc;
    if (flags & ~FRT_DEFORM_RECOMPUTE_NORMALS) return fail(FRT_ERR_INVALID_ARG, "animate_blend: unknown flag bits");
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate_blend: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigMeshes) return fail(FRT_ERR_INVALID_ARG, "animate_blend: binding " + std::to_string(binding) + " binds instances (frt_renderer_animate_instances_blend)");
    const std::string bad = check_blend_samples(n, samples, b->nclips);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_blend: " + bad);
    return pose_bound_meshes(r, "animate_blend", b, sample_list(n, samples), flags);
}

int frt_renderer_animate_cast(frt_renderer* r, uint32_t n, const frt_cast_entry* entries, uint32_t flags) {
    if (const int rc = check_entry(r, "animate_cast", kEditChecks | kRefit)) return rc;
    const std::vector<CastBinding> info = cast_bindings(r);
    const std::string bad = check_cast_entries(n, entries, flags, FRT_DEFORM_RECOMPUTE_NORMALS, info.data(), info.size(), r->rf.vert_count.size(), r->rf.inst.size());
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_cast: " + bad);
    std::vector<frt_clip_sample> samples(n);      // entry k: the list of one sample k
    std::vector<CastRange> ranges(n);
    for (uint32_t k = 0; k < n; ++k) { samples[k] = frt_clip_sample{entries[k].clip, entries[k].time, 1.0f, 0u}; ranges[k] = CastRange{k, 1u}; }
    return run_cast<CastEntry>(r, "animate_cast", n, entries, ranges.data(), info, n, samples.data(), flags);
}

int frt_renderer_animate_cast_blend(frt_renderer* r, uint32_t n, const frt_cast_blend_entry* entries, uint32_t nsamples, const frt_clip_sample* samples, uint32_t flags) {
    if (const int rc = check_entry(r, "animate_cast_blend", kEditChecks | kRefit)) return rc;
    const std::vector<CastBinding> info = cast_bindings(r);
    std::vector<frt_cast_entry> plain;
    const std::string bad = check_cast_blend_entries(n, entries, nsamples, samples, flags, FRT_DEFORM_RECOMPUTE_NORMALS, info.data(), info.size(), r->rf.vert_count.size(),
                                                     r->rf.inst.size(), plain);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_cast_blend: " + bad);
    std::vector<CastRange> ranges(n);
    for (uint32_t k = 0; k < n; ++k) ranges[k] = CastRange{entries[k].first_sample, entries[k].num_samples};
    return run_cast<CastEntry>(r, "animate_cast_blend", n, plain.data(), ranges.data(), info, nsamples, samples, flags);
}

// "Layering clips". The masks go into a buffer with room for FRT_MAX_RIG_MASKS of them, allocated at the binding's first call, so that every later set
// is one staged copy in stream order: an animate call enqueued before it reads the old values, one enqueued behind it the new ones, and the count a
// later layered call is checked against and launched with is the new one.
int frt_renderer_set_rig_masks(frt_renderer* r, uint32_t binding, uint32_t nmasks, const float* masks) {
    if (const int rc = check_entry(r, "set_rig_masks", kEditChecks | kRefit)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "set_rig_masks: unknown rig binding " + std::to_string(binding));
    const std::string bad = check_rig_masks(nmasks, masks, b->nnodes);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_rig_masks: " + bad);
    if (nmasks == 0) { b->nmasks = 0; return FRT_OK; }
    FRT_DEVICE(r);
    const uint32_t N = b->nnodes;
    const size_t bytes = (size_t)nmasks * N * 4;
    if (const int rc = b->masks.ensure(r, (size_t)FRT_MAX_RIG_MASKS * N * 4)) return rc;
    if (const int rc = r->rig_up.reserve(bytes, 0, r->stream)) return rc;
    float* up = reinterpret_cast<float*>(r->rig_up.h);
    for (uint32_t m = 0; m < nmasks; ++m)
        for (uint32_t i = 0; i < N; ++i) up[(size_t)m * N + b->place[i]] = masks[(size_t)m * N + i];
    HIP_TRY(hipMemcpyAsync(b->masks.p, r->rig_up.h, bytes, hipMemcpyHostToDevice, r->stream));
    if (const int rc = r->rig_up.mark(r->stream)) return rc;
    b->nmasks = nmasks;
    return FRT_OK;
}

// "Inverse kinematics". The goals go into a buffer [FRT_MAX_RIG_GOALS goals | enter [nnodes] | exit [nnodes]] and the targets into one of
// FRT_MAX_RIG_GOALS records, both allocated at the binding's first set_rig_goals with a goal, so that every later set is a staged copy in stream
// order: a layered call enqueued before it reads the old values, one enqueued behind it the new ones, and the count a later call launches with is
// the new one (a kernel argument, or a word of the cast's table). New goals are inert: the targets are reset to zero words, weight 0.
int frt_renderer_set_rig_goals(frt_renderer* r, uint32_t binding, uint32_t ngoals, const frt_rig_goal* goals) {
    if (const int rc = check_entry(r, "set_rig_goals", kEditChecks | kRefit)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "set_rig_goals: unknown rig binding " + std::to_string(binding));
    std::vector<frt_rig_goal> stored;
    const std::string bad = check_rig_goals(ngoals, goals, b->place, b->enter.data(), b->exit.data(), stored);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_rig_goals: " + bad);
    if (ngoals == 0) { b->ngoals = 0; b->goal_defs.clear(); return FRT_OK; }
    FRT_DEVICE(r);
    const uint32_t N = b->nnodes;
    const size_t def_bytes = sizeof(frt_rig_goal) * FRT_MAX_RIG_GOALS, bytes = def_bytes + (size_t)8 * N, target_bytes = sizeof(frt_rig_goal_target) * FRT_MAX_RIG_GOALS;
    if (const int rc = b->goals.ensure(r, bytes)) return rc;
    if (const int rc = b->goal_targets.ensure(r, target_bytes)) return rc;
    if (const int rc = r->rig_up.reserve(bytes, 0, r->stream)) return rc;
    memset(r->rig_up.h, 0, def_bytes);
    memcpy(r->rig_up.h, stored.data(), sizeof(frt_rig_goal) * ngoals);
    memcpy(r->rig_up.h + def_bytes, b->enter.data(), (size_t)4 * N);
    memcpy(r->rig_up.h + def_bytes + (size_t)4 * N, b->exit.data(), (size_t)4 * N);
    HIP_TRY(hipMemcpyAsync(b->goals.p, r->rig_up.h, bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipMemsetAsync(b->goal_targets.p, 0, target_bytes, r->stream));
    if (const int rc = r->rig_up.mark(r->stream)) return rc;
    b->ngoals = ngoals; b->goal_defs.swap(stored);
    return FRT_OK;
}

int frt_renderer_set_rig_goal_targets(frt_renderer* r, uint32_t binding, uint32_t ngoals, const frt_rig_goal_target* targets, uint32_t flags) {
    if (const int rc = check_entry(r, "set_rig_goal_targets", kEditChecks | kRefit)) return rc;
    if (flags & ~FRT_GOAL_TARGETS_DEVICE) return fail(FRT_ERR_INVALID_ARG, "set_rig_goal_targets: unknown flag bits");
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "set_rig_goal_targets: unknown rig binding " + std::to_string(binding));
    const size_t bytes = sizeof(frt_rig_goal_target) * (size_t)ngoals;
    if (flags & FRT_GOAL_TARGETS_DEVICE) {
        if (ngoals > FRT_MAX_RIG_GOALS || ngoals != b->ngoals) return fail(FRT_ERR_INVALID_ARG, "set_rig_goal_targets: " + std::to_string(ngoals) + " targets for " + std::to_string(b->ngoals) + " goals");
        if (ngoals && !targets) return fail(FRT_ERR_INVALID_ARG, "set_rig_goal_targets: null targets");
        if (ngoals == 0) return FRT_OK;
        if (const int rc = check_device_block(r, targets, bytes, 16, "set_rig_goal_targets", "targets", "FRT_GOAL_TARGETS_DEVICE")) return rc;
        FRT_DEVICE(r);
        HIP_TRY(hipMemcpyAsync(b->goal_targets.p, targets, bytes, hipMemcpyDeviceToDevice, r->stream));
        return FRT_OK;
    }
    const std::string bad = check_rig_goal_targets(ngoals, targets, b->ngoals, b->goal_defs.data());
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "set_rig_goal_targets: " + bad);
    if (ngoals == 0) return FRT_OK;
    FRT_DEVICE(r);
    if (const int rc = r->rig_up.reserve(bytes, 0, r->stream)) return rc;
    memcpy(r->rig_up.h, targets, bytes);
    HIP_TRY(hipMemcpyAsync(b->goal_targets.p, r->rig_up.h, bytes, hipMemcpyHostToDevice, r->stream));
    return r->rig_up.mark(r->stream);
}

int frt_renderer_animate_layers(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_layer* layers, uint32_t flags) {
    if (const int rc = check_entry(r, "animate_layers", kEditChecks | kRefit)) return rc;
    if (flags & ~FRT_DEFORM_RECOMPUTE_NORMALS) return fail(FRT_ERR_INVALID_ARG, "animate_layers: unknown flag bits");
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate_layers: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigMeshes) return fail(FRT_ERR_INVALID_ARG, "animate_layers: binding " + std::to_string(binding) + " binds instances (frt_renderer_animate_instances_layers)");
    const std::string bad = check_clip_layers(n, layers, b->nclips, b->nmasks);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_layers: " + bad);
    if (has_chain_goal(*b)) return pose_bound_meshes(r, "animate_layers", b, layer_list(n, layers, *b), flags, bound_goals<true>(*b));
    if (b->ngoals) return pose_bound_meshes(r, "animate_layers", b, layer_list(n, layers, *b), flags, bound_goals(*b));
    return pose_bound_meshes(r, "animate_layers", b, layer_list(n, layers, *b), flags);
}

int frt_renderer_animate_instances_layers(frt_renderer* r, uint32_t binding, uint32_t n, const frt_clip_layer* layers) {
    if (const int rc = check_entry(r, "animate_instances_layers", kEditChecks | kRefit)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "animate_instances_layers: unknown rig binding " + std::to_string(binding));
    if (b->kind != kRigInstances) return fail(FRT_ERR_INVALID_ARG, "animate_instances_layers: binding " + std::to_string(binding) + " binds meshes (frt_renderer_animate_layers)");
    const std::string bad = check_clip_layers(n, layers, b->nclips, b->nmasks);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_instances_layers: " + bad);
    if (has_chain_goal(*b)) return move_bound_instances(r, "animate_instances_layers", b, layer_list(n, layers, *b), bound_goals<true>(*b));
    if (b->ngoals) return move_bound_instances(r, "animate_instances_layers", b, layer_list(n, layers, *b), bound_goals(*b));
    return move_bound_instances(r, "animate_instances_layers", b, layer_list(n, layers, *b));
}

int frt_renderer_animate_cast_layers(frt_renderer* r, uint32_t n, const frt_cast_layers_entry* entries, uint32_t nlayers, const frt_clip_layer* layers, uint32_t flags) {
    if (const int rc = check_entry(r, "animate_cast_layers", kEditChecks | kRefit)) return rc;
    const std::vector<CastBinding> info = cast_bindings(r);
    std::vector<uint32_t> masks_of(r->rigs.size());
    for (size_t i = 0; i < r->rigs.size(); ++i) masks_of[i] = r->rigs[i].nmasks;
    std::vector<frt_cast_entry> plain;
    const std::string bad = check_cast_layers_entries(n, entries, nlayers, layers, flags, FRT_DEFORM_RECOMPUTE_NORMALS, info.data(), masks_of.data(), info.size(),
                                                      r->rf.vert_count.size(), r->rf.inst.size(), plain);
    if (!bad.empty()) return fail(FRT_ERR_INVALID_ARG, "animate_cast_layers: " + bad);
    std::vector<CastRange> ranges(n);
    for (uint32_t k = 0; k < n; ++k) ranges[k] = CastRange{entries[k].first_layer, entries[k].num_layers};
    bool goals = false, chain = false;      // the goal instantiation when any entry's binding carries goals; the chain one when any carries a chain
    for (uint32_t k = 0; k < n; ++k) { goals = goals || r->rigs[entries[k].binding].ngoals != 0; chain = chain || has_chain_goal(r->rigs[entries[k].binding]); }
    if (chain) return run_cast<CastLayersEntry, RigChainGoals>(r, "animate_cast_layers", n, plain.data(), ranges.data(), info, nlayers, layers, flags);
    if (goals) return run_cast<CastLayersEntry, RigBoundGoals>(r, "animate_cast_layers", n, plain.data(), ranges.data(), info, nlayers, layers, flags);
    return run_cast<CastLayersEntry>(r, "animate_cast_layers", n, plain.data(), ranges.data(), info, nlayers, layers, flags);
}

int frt_renderer_read_rig_pose(frt_renderer* r, uint32_t binding, float* joint_mats_out, float* morph_weights_out) {
    if (const int rc = check_entry(r, "read_rig_pose", kNotFailed)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b || b->kind != kRigMeshes) return fail(FRT_ERR_INVALID_ARG, "read_rig_pose: unknown rig binding " + std::to_string(binding));
    FRT_DEVICE(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (joint_mats_out && b->njoints) HIP_TRY(hipMemcpy(joint_mats_out, b->palette.p, (size_t)b->njoints * 64, hipMemcpyDeviceToHost));
    if (morph_weights_out && b->ntargets) HIP_TRY(hipMemcpy(morph_weights_out, b->weights.p, (size_t)b->ntargets * 4, hipMemcpyDeviceToHost));
    return FRT_OK;
}

int frt_renderer_unbind_rig(frt_renderer* r, uint32_t binding) {
    if (const int rc = check_entry(r, "unbind_rig", kNotFailed | kBetweenFrames)) return rc;
    RigBinding* b = find_binding(r, binding);
    if (!b) return fail(FRT_ERR_INVALID_ARG, "unbind_rig: unknown rig binding " + std::to_string(binding));
    FRT_DEVICE(r);
    b->release(r);
    *b = RigBinding();
    return FRT_OK;
}

} // extern "C"
