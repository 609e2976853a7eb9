// frt_rebuild.hip — kernels and driver of frt_renderer_rebuild_tree ("Rebuild"; frt_rebuild.hpp).
// Visibility between dependent steps comes from kernel boundaries on one stream, as in frt_refit.hip: no flags, no fences (per-XCD L2s are not
// coherent within a kernel). Indices are assigned by the sort and by scans, never by atomics: the result is a function of the device state alone.
// The only atomics are the min / max of the centroid bounds, which are exact and order-independent. No box arithmetic is written here: the boxes
// are the refit kernel's (frt_refit.hip), so every box is the padded union DESIGN.md §11 defines.
#include "frt_rebuild.hpp"
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace frt {

static const int kRbBlock = 256;
static const uint32_t kRbLeaf = 0x80000000u, kRbNone = 0xFFFFFFFFu;
static const uint32_t kRbBudget = (uint32_t)kStackDepth - 1u;      // build_quad_nodes: `budget`
// (The small results, RebuildScratch::words: frt_rebuild.hpp.)
static const int kLevelChunk = 16;      // binary levels assigned between two looks at the flags

// f32 bits whose unsigned order is the order of the floats (and back).
__device__ inline uint32_t ordered_bits(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ inline float ordered_float(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// Centroid of the bounds of the triangle the intersector sees (v0, v0 + e1, v0 + e2), as build_bvh2 takes it.
__device__ inline void slot_centroid(const SceneView& sc, uint32_t s, float c[3]) {
    const float4 v0 = sc.tris[3u * s], e1 = sc.tris[3u * s + 1u], e2 = sc.tris[3u * s + 2u];
    const float x[3] = {v0.x, v0.y, v0.z}, a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
    for (int k = 0; k < 3; ++k) {
        const float v1 = x[k] + a[k], v2 = x[k] + b[k];
        c[k] = 0.5f * (fminf(x[k], fminf(v1, v2)) + fmaxf(x[k], fmaxf(v1, v2)));
    }
}

// 1. Bounds of all centroids: a tree in LDS, then one atomic per block, axis and side (scene_extent_kernel's style).
__global__ void __launch_bounds__(kRbBlock) centroid_bounds_kernel(SceneView sc, uint32_t* words) {
    __shared__ float lo[3][kRbBlock], hi[3][kRbBlock];
    const uint32_t s = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    float c[3] = {__int_as_float(0x7F800000), __int_as_float(0x7F800000), __int_as_float(0x7F800000)};
    float d[3] = {-c[0], -c[1], -c[2]};
    if (s < sc.num_tris) { slot_centroid(sc, s, c); for (int k = 0; k < 3; ++k) d[k] = c[k]; }
    for (int k = 0; k < 3; ++k) { lo[k][threadIdx.x] = c[k]; hi[k][threadIdx.x] = d[k]; }
    __syncthreads();
    for (int w = kRbBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 3; ++k) {
                lo[k][threadIdx.x] = fminf(lo[k][threadIdx.x], lo[k][threadIdx.x + w]);
                hi[k][threadIdx.x] = fmaxf(hi[k][threadIdx.x], hi[k][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3u) {
        atomicMin(words + W_MIN + threadIdx.x, ordered_bits(lo[threadIdx.x][0]));
        atomicMax(words + W_MAX + threadIdx.x, ordered_bits(hi[threadIdx.x][0]));
    }
}

__device__ inline uint32_t spread10(uint32_t v) {      // bit i of a 10-bit value to bit 3i
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 2. One key per slot: 30-bit Morton code of the centroid inside the bounds << 32 | flattened triangle id. Ids are unique, so keys are.
__global__ void __launch_bounds__(kRbBlock) morton_keys_kernel(SceneView sc, const uint32_t* words, unsigned long long* keys) {
    const uint32_t s = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (s >= sc.num_tris) return;
    float c[3];
    slot_centroid(sc, s, c);
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = ordered_float(words[W_MIN + k]), ext = ordered_float(words[W_MAX + k]) - lo;
        const float g = ext > 0.0f ? (c[k] - lo) * (1024.0f / ext) : 0.0f;
        q[k] = (uint32_t)fminf(fmaxf(g, 0.0f), 1023.0f);      // (fmaxf drops a NaN)
    }
    const uint32_t code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    keys[s] = ((unsigned long long)code << 32) | (unsigned long long)__float_as_uint(sc.tris[3u * s].w);
}

// 4. Slot s of the new order takes the triangle whose key sorted to place s; the id -> slot table follows.
__global__ void __launch_bounds__(kRbBlock) gather_slots_kernel(SceneView sc, const uint32_t* slot_of, const unsigned long long* keys, float4* tris, uint32_t* new_slot_of) {
    const uint32_t s = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (s >= sc.num_tris) return;
    const uint32_t id = (uint32_t)(keys[s] & 0xFFFFFFFFull);
    if (id >= sc.num_tris) return;
    const uint32_t from = slot_of[id];
    if (from >= sc.num_tris) return;
    for (uint32_t k = 0; k < 3u; ++k) tris[3u * s + k] = sc.tris[3u * from + k];
    new_slot_of[id] = s;
}

// 5. Karras (2012): inner node i of the binary radix tree over the leaves' first keys (leaf j = slots 2j, 2j + 1: key 2j). A child reference is
// an inner node's index or kRbLeaf | leaf index.
__device__ inline int common_prefix(const unsigned long long* keys, int leaves, int i, int j) {
    if (j < 0 || j >= leaves) return -1;
    return __clzll((long long)(keys[2 * (size_t)i] ^ keys[2 * (size_t)j]));
}
__global__ void __launch_bounds__(kRbBlock) radix_tree_kernel(const unsigned long long* keys, uint32_t leaves, uint32_t* left, uint32_t* right) {
    const uint32_t g = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (g + 1u >= leaves) return;
    const int i = (int)g, n = (int)leaves;
    const int d = common_prefix(keys, n, i, i + 1) > common_prefix(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = common_prefix(keys, n, i, i - d);
    int lmax = 2;
    while (common_prefix(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2) if (common_prefix(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d, dnode = common_prefix(keys, n, i, j);
    int s = 0;
    for (int t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (common_prefix(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int split = i + s * d + (d < 0 ? -1 : 0), first = i < j ? i : j, last = i < j ? j : i;
    left[g] = first == split ? (kRbLeaf | (uint32_t)split) : (uint32_t)split;
    right[g] = last == split + 1 ? (kRbLeaf | (uint32_t)(split + 1)) : (uint32_t)(split + 1);
}

// 6a. Levels of the binary tree, top-down: the nodes of level `cur` give their inner children level cur + 1.
__global__ void __launch_bounds__(kRbBlock) binary_level_kernel(const uint32_t* left, const uint32_t* right, uint32_t inner, uint32_t cur, uint32_t* level, uint32_t* words) {
    const uint32_t i = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (i >= inner || level[i] != cur) return;
    const uint32_t c[2] = {left[i], right[i]};
    for (int k = 0; k < 2; ++k)
        if (!(c[k] & kRbLeaf) && c[k] < inner) { level[c[k]] = cur + 1u; words[W_FLAGS + cur + 1u] = 1u; }
}
// 6b. Heights of the binary subtrees (a leaf = 1), bottom-up: level `cur`, every deeper level done.
__global__ void __launch_bounds__(kRbBlock) binary_height_kernel(const uint32_t* left, const uint32_t* right, const uint32_t* level, uint32_t inner, uint32_t cur, uint32_t* height) {
    const uint32_t i = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (i >= inner || level[i] != cur) return;
    const uint32_t c[2] = {left[i], right[i]};
    uint32_t h = 1u;
    for (int k = 0; k < 2; ++k) if (!(c[k] & kRbLeaf) && c[k] < inner) h = max(h, height[c[k]]);
    height[i] = h + 1u;
}

// build_quad_nodes's `fits`: with `used` entries pushed by the ancestors, may a node hold these children and still finish every inner child as a
// plain binary subtree inside the budget?
__device__ inline bool fold_fits(const uint32_t* c, int n, uint32_t used, const uint32_t* height, uint32_t inner) {
    if (used + (uint32_t)(n - 1) > kRbBudget) return false;
    for (int i = 0; i < n; ++i)
        if (!(c[i] & kRbLeaf) && c[i] < inner && used + (uint32_t)(n - 1) + (height[c[i]] - 1u) > kRbBudget) return false;
    return true;
}
// Child i of the set c[0..n) replaced by its own two children, when the larger set still fits (fold_fits).
__device__ inline bool fold_expand(uint32_t* c, int n, int i, uint32_t used, const uint32_t* left, const uint32_t* right, const uint32_t* height, uint32_t inner) {
    uint32_t w[4] = {c[0], c[1], c[2], c[3]};
    for (int k = n; k > i + 1; --k) w[k] = w[k - 1];
    w[i] = left[c[i]]; w[i + 1] = right[c[i]];
    if (!fold_fits(w, n + 1, used, height, inner)) return false;
    for (int k = 0; k < 4; ++k) c[k] = w[k];
    return true;
}
// The plain mode's order: inner children are replaced left to right, pass after pass, while the set still fits (topological, no boxes).
__device__ inline int fold_left_to_right(uint32_t* c, int n, uint32_t used, const uint32_t* left, const uint32_t* right, const uint32_t* height, uint32_t inner) {
    bool grew = true, stop = false;
    while (grew && !stop && n < 4) {
        grew = false;
        for (int i = 0; i < n && n < 4 && !stop;) {
            if ((c[i] & kRbLeaf) || c[i] >= inner) { ++i; continue; }
            if (!fold_expand(c, n, i, used, left, right, height, inner)) { stop = true; break; }
            ++n; i += 2; grew = true;
        }
    }
    return n;
}
// The refined mode's order, build_quad_nodes's greedy fold: the inner child with the largest half-area (nbox: one box per binary inner node) is
// replaced first, ties to the lower child position, until nothing is left to replace or the set no longer fits.
__device__ inline float fold_half_area(const float* nbox, uint32_t b) {
    const float* x = nbox + (size_t)b * 6u;
    const float dx = x[3] - x[0], dy = x[4] - x[1], dz = x[5] - x[2];
    return dx * dy + dy * dz + dz * dx;
}
__device__ inline int fold_by_area(uint32_t* c, int n, uint32_t used, const uint32_t* left, const uint32_t* right, const uint32_t* height, uint32_t inner, const float* nbox) {
    while (n < 4) {
        int pick = -1; float best = -1.0f;
        for (int i = 0; i < n; ++i) {
            if ((c[i] & kRbLeaf) || c[i] >= inner) continue;
            const float a = fold_half_area(nbox, c[i]);
            if (a > best) { best = a; pick = i; }
        }
        if (pick < 0 || !fold_expand(c, n, pick, used, left, right, height, inner)) break;
        ++n;
    }
    return n;
}
// 6c. One level of the fold: quad node base + t is the binary node front[t]. It takes that node's two children and folds further ones in, by area
// with `nbox`, else left to right. Writes the whole node: far-away point boxes, the children as BINARY references (quad_number_kernel turns them
// into quad ones), and how many of them are inner.
__global__ void __launch_bounds__(kRbBlock) quad_fold_kernel(const uint32_t* left, const uint32_t* right, const uint32_t* height, uint32_t inner, const uint32_t* front,
                                                             const uint32_t* used, uint32_t m, uint32_t base, uint32_t cap, float4* nodes, uint32_t* cnt, const float* nbox) {
    const uint32_t t = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (t >= m || base + t >= cap) return;
    const uint32_t b = front[t], u = used[t];
    uint32_t c[4] = {kRbNone, kRbNone, kRbNone, kRbNone};
    int n = 0;
    if (b < inner) {
        c[0] = left[b]; c[1] = right[b];
        n = nbox ? fold_by_area(c, 2, u, left, right, height, inner, nbox) : fold_left_to_right(c, 2, u, left, right, height, inner);
    }
    uint32_t k_inner = 0;
    for (int i = 0; i < n; ++i) if (!(c[i] & kRbLeaf)) ++k_inner;
    float4* q = nodes + (size_t)(base + t) * 8u;
    const float4 far = make_float4(1.0e30f, 1.0e30f, 1.0e30f, 1.0e30f);      // empty slot: a far-away point (build_quad_nodes); the refit leaves it alone
    for (int k = 0; k < 6; ++k) q[k] = far;
    q[6] = make_float4(__uint_as_float(c[0]), __uint_as_float(c[1]), __uint_as_float(c[2]), __uint_as_float(c[3]));
    q[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    cnt[t] = k_inner;
}
// 6d. Breadth-first numbers from the exclusive scan of the inner-child counts: the k-th inner child of the level becomes quad node next_base + k and
// entry k of the next frontier. Leaves become kLeafFlag | count << 24 | first slot (leaf j = slots 2j, 2j + 1; the last one may hold one slot).
__global__ void __launch_bounds__(kRbBlock) quad_number_kernel(const uint32_t* used, const uint32_t* cnt, const uint32_t* off, uint32_t m, uint32_t base, uint32_t cap,
                                                               uint32_t num_tris, float4* nodes, uint32_t* next_front, uint32_t* next_used, uint32_t next_cap, uint32_t* words) {
    const uint32_t t = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (t >= m || base + t >= cap) return;
    float4* q = nodes + (size_t)(base + t) * 8u;
    const float4 r = q[6];
    uint32_t c[4] = {__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), __float_as_uint(r.w)};
    uint32_t n = 0;
    for (int i = 0; i < 4; ++i) if (c[i] != kRbNone) ++n;
    uint32_t o = off[t];
    for (int i = 0; i < 4; ++i) {
        if (c[i] == kRbNone) continue;
        if (c[i] & kRbLeaf) {
            const uint32_t first = 2u * (c[i] & 0x7FFFFFFFu);
            c[i] = kRbLeaf | ((first + 1u < num_tris ? 2u : 1u) << 24) | first;
        } else {
            if (o < next_cap) { next_front[o] = c[i]; next_used[o] = used[t] + (n - 1u); }
            c[i] = base + m + o;
            ++o;
        }
    }
    q[6] = make_float4(__uint_as_float(c[0]), __uint_as_float(c[1]), __uint_as_float(c[2]), __uint_as_float(c[3]));
    if (t == m - 1u) words[W_NEXT] = off[t] + cnt[t];
}
// A tree that is a lone leaf (at most two triangles): one quad node with one child, as build_quad_nodes makes it.
__global__ void lone_leaf_kernel(uint32_t num_tris, float4* nodes) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float4 far = make_float4(1.0e30f, 1.0e30f, 1.0e30f, 1.0e30f);
    for (int k = 0; k < 6; ++k) nodes[k] = far;
    nodes[6] = make_float4(__uint_as_float(kRbLeaf | (num_tris << 24)), __uint_as_float(kRbNone), __uint_as_float(kRbNone), __uint_as_float(kRbNone));
    nodes[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// 8. Deepest traversal stack below a node, bottom-up: (children - 1) + max over inner children (build_quad_nodes: `need`).
__global__ void __launch_bounds__(kRbBlock) stack_need_kernel(const float4* nodes, uint32_t q0, uint32_t q1, uint32_t num, uint32_t* need) {
    const uint32_t i = q0 + blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (i >= q1 || i >= num) return;
    const float4 r = nodes[(size_t)i * 8u + 6u];
    const uint32_t c[4] = {__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), __float_as_uint(r.w)};
    uint32_t n = 0, deepest = 0;
    for (int k = 0; k < 4; ++k) {
        if (c[k] == kRbNone) continue;
        ++n;
        if (!(c[k] & kRbLeaf) && c[k] < num) deepest = max(deepest, need[c[k]]);
    }
    need[i] = (n > 0u ? n - 1u : 0u) + deepest;
}

static inline dim3 grid_for(uint32_t n) { return dim3((n + kRbBlock - 1) / kRbBlock); }
static inline size_t align256(size_t n) { return (n + 255u) & ~(size_t)255u; }

void rebuild_release(RebuildScratch& s) {
    if (s.base) (void)hipFree(s.base);
    if (s.ploc.base) (void)hipFree(s.ploc.base);
    if (s.h_words) (void)hipHostFree(s.h_words);
    s = RebuildScratch{};
}

hipError_t rebuild_reserve(RebuildScratch& s, uint32_t num_tris) {
    if (s.base && s.cap_tris >= num_tris) return hipSuccess;
    rebuild_release(s);
    const uint32_t inner = rebuild_max_nodes(num_tris);
    hipError_t e;
    rocprim::double_buffer<unsigned long long> kb(nullptr, nullptr);
    // (the scratch may serve scenes of fewer triangles than it was reserved for, DESIGN.md §14, and the sort picks its algorithm by size: room for the
    // largest need at every halving down from num_tris; rebuild_tree checks the need of the size it sorts against this before it sorts)
    for (size_t n = num_tris; n > 0; n /= 2) {
        size_t need = 0;
        if ((e = rocprim::radix_sort_keys(nullptr, need, kb, n, 0u, 64u, (hipStream_t) nullptr)) != hipSuccess) return e;
        s.sort_bytes = std::max(s.sort_bytes, need);
    }
    if ((e = rocprim::exclusive_scan(nullptr, s.scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)inner, rocprim::plus<uint32_t>(), (hipStream_t) nullptr)) != hipSuccess) return e;
    const size_t kbytes = align256((size_t)num_tris * 8u), ibytes = align256((size_t)inner * 4u);
    const size_t total = 2u * kbytes + align256(s.sort_bytes) + align256(s.scan_bytes) + 11u * ibytes + align256(kRebuildWords * 4u);
    if ((e = hipMalloc(&s.base, total)) != hipSuccess) { s = RebuildScratch{}; return e; }
    if ((e = hipHostMalloc((void**)&s.h_words, kRebuildWords * 4u)) != hipSuccess) { rebuild_release(s); return e; }
    uint8_t* p = (uint8_t*)s.base;
    auto take = [&](size_t n) { uint8_t* r = p; p += n; return r; };
    s.keys[0] = (unsigned long long*)take(kbytes); s.keys[1] = (unsigned long long*)take(kbytes);
    s.sort_tmp = take(align256(s.sort_bytes)); s.scan_tmp = take(align256(s.scan_bytes));
    uint32_t** per_inner[11] = {&s.left, &s.right, &s.level, &s.height, &s.front[0], &s.front[1], &s.used[0], &s.used[1], &s.cnt, &s.off, &s.need};
    for (uint32_t** q : per_inner) *q = (uint32_t*)take(ibytes);
    s.words = (uint32_t*)take(align256(kRebuildWords * 4u));
    s.bytes = total; s.cap_tris = num_tris; s.cap_inner = inner;
    return hipSuccess;
}

#define RB_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

hipError_t rebuild_fetch_words(RebuildScratch& s, hipStream_t stream) {
    RB_TRY(hipMemcpyAsync(s.h_words, s.words, kRebuildWords * 4u, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// 5 - 8 for one topology: `sah` builds the refined binary tree (frt_ploc.hip; its root is the last inner node made) and folds by area, else
// Karras's radix tree (root: inner node 0) and the left-to-right fold. res.num_nodes == 0: the tree could not be numbered; res.fell_back != 0
// (refined mode only): this topology must not be used.
static hipError_t build_nodes(RebuildScratch& s, const SceneView& cur, const unsigned long long* keys, const RebuildTarget& out, unsigned int* ext, hipStream_t stream, bool sah, RebuildResult& res) {
    const uint32_t N = cur.num_tris, leaves = (N + 1u) / 2u, inner = leaves - 1u, cap = rebuild_max_nodes(N);
    res.num_nodes = 0; res.stack_need = 0;
    res.levels.assign(1, 0u);
    uint32_t total = 0;
    if (inner == 0) {
        hipLaunchKernelGGL(lone_leaf_kernel, dim3(1), dim3(64), 0, stream, N, out.nodes);
        RB_TRY(hipGetLastError());
        total = 1; res.levels.push_back(1u);
    } else {
        // 5: binary topology
        uint32_t root = 0;
        if (sah) {
            bool ok = false;
            RB_TRY(ploc_topology(s, out.tris, N, stream, res.iterations, ok));
            if (!ok) { res.fell_back = 1u; return hipSuccess; }
            root = inner - 1u;
        } else
            hipLaunchKernelGGL(radix_tree_kernel, grid_for(inner), dim3(kRbBlock), 0, stream, keys, leaves, s.left, s.right);
        // 6a: levels, a chunk of launches between two looks at the flags
        RB_TRY(hipMemsetAsync(s.level, 0xFF, (size_t)inner * 4u, stream));
        RB_TRY(hipMemsetAsync(s.level + root, 0, 4u, stream));
        uint32_t blevels = 0;
        for (uint32_t c0 = 0; c0 < (uint32_t)kMaxBinaryLevels && blevels == 0; c0 += (uint32_t)kLevelChunk) {
            for (uint32_t l = c0; l < c0 + (uint32_t)kLevelChunk; ++l)
                hipLaunchKernelGGL(binary_level_kernel, grid_for(inner), dim3(kRbBlock), 0, stream, s.left, s.right, inner, l, s.level, s.words);
            RB_TRY(hipGetLastError());
            RB_TRY(rebuild_fetch_words(s, stream));
            for (uint32_t l = c0 + 1u; l <= c0 + (uint32_t)kLevelChunk; ++l)
                if (!s.h_words[W_FLAGS + l]) { blevels = l; break; }
        }
        if (blevels == 0) { if (sah) res.fell_back = 2u; return hipSuccess; }      // deeper than 64 levels (Morton: than 64-bit keys allow): res.num_nodes stays 0
        // 6b: heights, deepest level first
        for (uint32_t l = blevels; l-- > 0;)
            hipLaunchKernelGGL(binary_height_kernel, grid_for(inner), dim3(kRbBlock), 0, stream, s.left, s.right, s.level, inner, l, s.height);
        RB_TRY(hipGetLastError());
        // 6c, 6d: the fold, one quad level per round; the root has nothing pushed above it
        RB_TRY(hipMemsetD32Async((hipDeviceptr_t)s.front[0], (int)root, 1u, stream));
        RB_TRY(hipMemsetAsync(s.used[0], 0, 4u, stream));
        uint32_t m = 1, base = 0; int f = 0;
        while (m > 0) {
            if (base + m > cap) return hipSuccess;
            hipLaunchKernelGGL(quad_fold_kernel, grid_for(m), dim3(kRbBlock), 0, stream, s.left, s.right, s.height, inner, s.front[f], s.used[f], m, base, cap, out.nodes, s.cnt,
                               sah ? (const float*)s.ploc.nbox : (const float*)nullptr);
            RB_TRY(hipGetLastError());
            size_t scan_bytes = s.scan_bytes;
            RB_TRY(rocprim::exclusive_scan(s.scan_tmp, scan_bytes, s.cnt, s.off, 0u, (size_t)m, rocprim::plus<uint32_t>(), stream));
            hipLaunchKernelGGL(quad_number_kernel, grid_for(m), dim3(kRbBlock), 0, stream, s.used[f], s.cnt, s.off, m, base, cap, N, out.nodes, s.front[f ^ 1], s.used[f ^ 1], s.cap_inner, s.words);
            RB_TRY(hipGetLastError());
            RB_TRY(rebuild_fetch_words(s, stream));
            base += m; res.levels.push_back(base);
            m = s.h_words[W_NEXT]; f ^= 1;
        }
        total = base;
    }
    // 7, 8: boxes by the refit kernel (scene extent first, for the pad) and the stack need, deepest level first
    SceneView nv = cur;
    nv.tris = out.tris; nv.nodes4 = out.nodes; nv.num_nodes4 = total;
    const RefitArgs none{nullptr, 0u, 0u, nullptr, nullptr, ext};
    RB_TRY(launch_instance_transform(nv, none, stream));
    for (size_t l = res.levels.size() - 1; l-- > 0;) {
        const uint32_t q0 = res.levels[l], q1 = res.levels[l + 1];
        RB_TRY(launch_refit_level(nv, ext, 0u, 0u, q0, q1, stream));
        hipLaunchKernelGGL(stack_need_kernel, grid_for(q1 - q0), dim3(kRbBlock), 0, stream, out.nodes, q0, q1, total, s.need);
    }
    RB_TRY(hipGetLastError());
    RB_TRY(hipMemcpyAsync(s.h_words, s.need, 4u, hipMemcpyDeviceToHost, stream));
    RB_TRY(hipStreamSynchronize(stream));
    res.stack_need = s.h_words[0];
    res.num_nodes = total;
    return hipSuccess;
}

hipError_t rebuild_tree(RebuildScratch& s, const SceneView& cur, const uint32_t* slot_of, const RebuildTarget& out, unsigned int* ext, hipStream_t stream, RebuildResult& res, uint32_t mode) {
    res = RebuildResult{};
    const uint32_t N = cur.num_tris;
    if (N == 0 || N > s.cap_tris) return hipErrorInvalidValue;
    // 1-4: bounds, keys, sort, gather
    RB_TRY(hipMemsetAsync(s.words, 0, kRebuildWords * 4u, stream));
    RB_TRY(hipMemsetAsync(s.words + W_MIN, 0xFF, 3u * 4u, stream));
    hipLaunchKernelGGL(centroid_bounds_kernel, grid_for(N), dim3(kRbBlock), 0, stream, cur, s.words);
    hipLaunchKernelGGL(morton_keys_kernel, grid_for(N), dim3(kRbBlock), 0, stream, cur, s.words, s.keys[0]);
    RB_TRY(hipGetLastError());
    rocprim::double_buffer<unsigned long long> kb(s.keys[0], s.keys[1]);
    size_t sort_bytes = 0;
    RB_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, kb, (size_t)N, 0u, 64u, stream));
    if (sort_bytes > s.sort_bytes) return hipErrorOutOfMemory;      // (never seen: rebuild_reserve)
    sort_bytes = s.sort_bytes;
    RB_TRY(rocprim::radix_sort_keys(s.sort_tmp, sort_bytes, kb, (size_t)N, 0u, 64u, stream));
    const unsigned long long* keys = kb.current();
    hipLaunchKernelGGL(gather_slots_kernel, grid_for(N), dim3(kRbBlock), 0, stream, cur, slot_of, keys, out.tris, out.slot_of);
    RB_TRY(hipGetLastError());
    if (mode != 0u && N > 2u) {
        // the refined tree; it is kept when it is complete and fits the traversal stack
        RB_TRY(build_nodes(s, cur, keys, out, ext, stream, true, res));
        if (!res.fell_back && res.num_nodes > 0 && res.stack_need > kRbBudget) res.fell_back = 2u;
        if (!res.fell_back && res.num_nodes > 0) { res.origin = 2u; return hipSuccess; }
        if (!res.fell_back) res.fell_back = 2u;
        RB_TRY(hipMemsetAsync(s.words + W_NEXT, 0, (kRebuildWords - W_NEXT) * 4u, stream));      // the level flags and the frontier size, as a Morton-mode call finds them
    }
    RB_TRY(build_nodes(s, cur, keys, out, ext, stream, false, res));
    res.origin = mode != 0u && N <= 2u ? 2u : 1u;      // (a lone leaf is one node in either mode)
    return hipSuccess;
}

} // namespace frt
