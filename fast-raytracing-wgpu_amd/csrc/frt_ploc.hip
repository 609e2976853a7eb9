// frt_ploc.hip — the binary topology of the refined rebuild mode (FRT_REBUILD_SAH; DESIGN.md §11, "Refined rebuild"; frt_rebuild.hpp): parallel
// locally-ordered clustering (Meister and Bittner, 2018) over the leaves in Morton order. Every iteration each cluster finds its nearest neighbour
// among the kPlocRadius clusters on either side (distance: half-area of the union box), mutual nearest neighbours merge into a new inner node that
// takes the lower one's place, and the array is compacted in order. As in frt_rebuild.hip, indices come from scans, never from atomics, and
// visibility between steps comes from kernel boundaries on one stream (per-XCD L2s are not coherent within a kernel): no flags, no fences.
#include "frt_rebuild.hpp"
#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_scan.hpp>

namespace frt {

static const int kPlocBlock = 256;
static const uint32_t kPlocLeaf = 0x80000000u, kPlocNone = 0xFFFFFFFFu;
// Search radius. Measured at 8, 16 and 32 on the three timing scenes (profiles/r7_experiments/tree_rebuild_sah.md): 8 gives the best frame time on the
// 82k blob and the colonnade (4.77 / 4.85 / 4.95 ms and 7.90 / 8.24 / 8.51 ms), the Cornell Box is within 1 % at all three, and the call is the fastest.
#ifndef FRT_PLOC_RADIUS
#define FRT_PLOC_RADIUS 8
#endif
static const int kPlocRadius = FRT_PLOC_RADIUS;
// The tail kernel takes over when the cluster array fits one workgroup: one cluster per thread of the largest workgroup (1024). Its LDS: six box
// planes (24 KiB), ids and neighbours (8 KiB) and the block scan's storage, about 40 KiB of the 64 KiB a workgroup may declare statically.
static const int kPlocTail = 1024;
// Iterations between two looks at the live count while the array is larger than that.
static const int kPlocChunk = 4;
// Bound on the iterations: kPlocIterFactor * ceil(log2(leaves)). Seen on the test and timing scenes (radius 8 / 16): Cornell Box, 660 leaves, 30 - 37
// iterations, up to 3.7 per log2(leaves); ReSTIR scene 35 - 36; 82k blob, 41k leaves, 47 / 49 (3.1); colonnade, 123k leaves, 49 / 53 (3.1); 151
// coincident leaves 8. So 8 leaves a little more than twice the largest ratio seen. Input that merges one pair per iteration (geometric spacing) and
// has more than 8 * ceil(log2(leaves)) leaves passes it and gets the Morton tree.
static const uint32_t kPlocIterFactor = 8u;

static uint32_t ploc_max_iterations(uint32_t leaves) {
    uint32_t lg = 1u;
    while (lg < 32u && (1u << lg) < leaves) ++lg;
    return kPlocIterFactor * lg;
}

struct PlocBox { float lo[3], hi[3]; };

__device__ inline PlocBox ploc_union(const PlocBox& a, const PlocBox& b) {
    PlocBox u;
    for (int k = 0; k < 3; ++k) { u.lo[k] = fminf(a.lo[k], b.lo[k]); u.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
    return u;
}
// Half-area of the union box, one fixed expression: d(a, b) == d(b, a). A NaN (inf * 0) counts as +inf, so the order below stays total.
__device__ inline float ploc_distance(const PlocBox& a, const PlocBox& b) {
    const PlocBox u = ploc_union(a, b);
    const float dx = u.hi[0] - u.lo[0], dy = u.hi[1] - u.lo[1], dz = u.hi[2] - u.lo[2];
    const float d = dx * dy + dy * dz + dz * dx;
    return d == d ? d : __int_as_float(0x7F800000);
}
// The tie rule: is pair (i, j) with distance d before pair (i, bj) with distance bd under the key (d, j != (i ^ 1), |i - j|, min(i, j))? The key is
// the same from both ends of a pair and differs between any two pairs, so the globally smallest pair is chosen from both ends and merges.
__device__ inline bool ploc_before(uint32_t i, float d, uint32_t j, float bd, uint32_t bj) {
    if (bj == kPlocNone) return true;
    if (d != bd) return d < bd;
    const uint32_t s = j != (i ^ 1u), bs = bj != (i ^ 1u);
    if (s != bs) return s < bs;
    const uint32_t w = j > i ? j - i : i - j, bw = bj > i ? bj - i : i - bj;
    if (w != bw) return w < bw;
    return min(i, j) < min(i, bj);
}

// Leaf boxes: leaf j = slots 2j and 2j + 1 (the last may hold one), the f32 bounds of the triangles the intersector sees, as slot_centroid reads them.
__global__ void __launch_bounds__(kPlocBlock) ploc_leaf_kernel(const float4* tris, uint32_t num_tris, uint32_t leaves, uint32_t cap, float* cbox, uint32_t* cid, uint32_t* words) {
    const uint32_t j = blockIdx.x * (uint32_t)kPlocBlock + threadIdx.x;
    if (j == 0u) { words[W_PCOUNT] = leaves; words[W_PNODES] = 0u; words[W_PITERS] = 0u; words[W_PFAIL] = 0u; }
    if (j >= leaves) return;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = __int_as_float(0x7F800000); hi[k] = -lo[k]; }
    for (uint32_t s = 2u * j; s < 2u * j + 2u && s < num_tris; ++s) {
        const float4 v0 = tris[3u * s], e1 = tris[3u * s + 1u], e2 = tris[3u * s + 2u];
        const float x[3] = {v0.x, v0.y, v0.z}, a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
        for (int k = 0; k < 3; ++k) {
            const float v1 = x[k] + a[k], v2 = x[k] + b[k];
            lo[k] = fminf(lo[k], fminf(x[k], fminf(v1, v2)));
            hi[k] = fmaxf(hi[k], fmaxf(x[k], fmaxf(v1, v2)));
        }
    }
    for (int k = 0; k < 3; ++k) { cbox[(size_t)k * cap + j] = lo[k]; cbox[(size_t)(3 + k) * cap + j] = hi[k]; }
    cid[j] = kPlocLeaf | j;
}

// Nearest neighbour of cluster i among i - R .. i + R. The block's boxes and a halo of R on each side are staged in LDS once.
__global__ void __launch_bounds__(kPlocBlock) ploc_nn_kernel(const float* cbox, uint32_t cap, const uint32_t* words, uint32_t parity, uint32_t* nn) {
    __shared__ float sb[6][kPlocBlock + 2 * kPlocRadius];
    const uint32_t n = min(words[W_PCOUNT + parity], cap);
    const uint32_t b0 = blockIdx.x * (uint32_t)kPlocBlock;
    if (b0 >= n) return;
    for (uint32_t t = threadIdx.x; t < (uint32_t)(kPlocBlock + 2 * kPlocRadius); t += (uint32_t)kPlocBlock) {
        const long long g = (long long)b0 - kPlocRadius + (long long)t;
        if (g >= 0 && g < (long long)n)
            for (int k = 0; k < 6; ++k) sb[k][t] = cbox[(size_t)k * cap + (size_t)g];
    }
    __syncthreads();
    const uint32_t i = b0 + threadIdx.x;
    if (i >= n) return;
    const uint32_t li = threadIdx.x + (uint32_t)kPlocRadius;
    PlocBox me;
    for (int k = 0; k < 3; ++k) { me.lo[k] = sb[k][li]; me.hi[k] = sb[3 + k][li]; }
    const uint32_t j0 = i > (uint32_t)kPlocRadius ? i - (uint32_t)kPlocRadius : 0u, j1 = min(n - 1u, i + (uint32_t)kPlocRadius);
    uint32_t best = kPlocNone; float bd = 0.0f;
    for (uint32_t j = j0; j <= j1; ++j) {
        if (j == i) continue;
        const uint32_t lj = j - b0 + (uint32_t)kPlocRadius;
        PlocBox o;
        for (int k = 0; k < 3; ++k) { o.lo[k] = sb[k][lj]; o.hi[k] = sb[3 + k][lj]; }
        const float d = ploc_distance(me, o);
        if (ploc_before(i, d, j, bd, best)) { best = j; bd = d; }
    }
    nn[i] = best;
}

// Merge and keep flags, packed for one scan: bit 0, i merges with j = nn[i] (nn[j] == i and i < j); bit 32, i stays in the array (it is not the
// upper half of a merging pair). Zero beyond the live count, up to the `bound` the scan runs over.
__global__ void __launch_bounds__(kPlocBlock) ploc_flag_kernel(const uint32_t* nn, const uint32_t* words, uint32_t parity, uint32_t cap, uint32_t bound, unsigned long long* flag) {
    const uint32_t i = blockIdx.x * (uint32_t)kPlocBlock + threadIdx.x;
    if (i >= bound || i >= cap) return;
    const uint32_t n = min(words[W_PCOUNT + parity], cap);
    unsigned long long f = 0ull;
    if (i < n) {
        const uint32_t j = nn[i];
        const bool mutual = j < n && nn[j] == i;
        f = (mutual && i < j ? 1ull : 0ull) | (mutual && i > j ? 0ull : (1ull << 32));
    }
    flag[i] = f;
}

// Writes the new inner nodes and the compacted array: the node numbers continue from the nodes made so far by the exclusive scan of the merge flags,
// the places come from the exclusive scan of the keep flags. The last live thread hands the new counts to the next iteration.
__global__ void __launch_bounds__(kPlocBlock) ploc_merge_kernel(const float* cbox, const uint32_t* cid, const uint32_t* nn, const unsigned long long* flag, const unsigned long long* scan,
                                                                  uint32_t cap, uint32_t inner, uint32_t* words, uint32_t parity, float* obox, uint32_t* oid,
                                                                  uint32_t* left, uint32_t* right, float* nbox) {
    const uint32_t i = blockIdx.x * (uint32_t)kPlocBlock + threadIdx.x;
    const uint32_t n = min(words[W_PCOUNT + parity], cap), made = words[W_PNODES + parity];
    if (i >= n) return;
    const unsigned long long f = flag[i], s = scan[i];
    const uint32_t merge = (uint32_t)(f & 1ull), keep = (uint32_t)(f >> 32), node = made + (uint32_t)(s & 0xFFFFFFFFull), dest = (uint32_t)(s >> 32);
    if (i == n - 1u) {
        words[W_PCOUNT + (parity ^ 1u)] = dest + keep;
        words[W_PNODES + (parity ^ 1u)] = node + merge;
        if (n > 1u) words[W_PITERS] = words[W_PITERS] + 1u;      // (one writer per kernel)
    }
    if (!keep || dest >= cap) return;
    PlocBox me;
    for (int k = 0; k < 3; ++k) { me.lo[k] = cbox[(size_t)k * cap + i]; me.hi[k] = cbox[(size_t)(3 + k) * cap + i]; }
    uint32_t id = cid[i];
    if (merge && node < inner) {
        const uint32_t j = nn[i];
        PlocBox o;
        for (int k = 0; k < 3; ++k) { o.lo[k] = cbox[(size_t)k * cap + j]; o.hi[k] = cbox[(size_t)(3 + k) * cap + j]; }
        me = ploc_union(me, o);
        left[node] = id; right[node] = cid[j];
        for (int k = 0; k < 3; ++k) { nbox[(size_t)node * 6u + k] = me.lo[k]; nbox[(size_t)node * 6u + 3u + k] = me.hi[k]; }
        id = node;
    }
    for (int k = 0; k < 3; ++k) { obox[(size_t)k * cap + dest] = me.lo[k]; obox[(size_t)(3 + k) * cap + dest] = me.hi[k]; }
    oid[dest] = id;
}

// The tail: the array fits one workgroup, so every remaining iteration (search, merge, scan, compaction) runs here in LDS with __syncthreads between
// the steps, to the root. The same rule as the three kernels above: where the tail begins does not change the tree.
__global__ void __launch_bounds__(kPlocTail) ploc_tail_kernel(const float* cbox, const uint32_t* cid, uint32_t cap, uint32_t inner, uint32_t* words, uint32_t parity,
                                                              uint32_t max_iters, uint32_t* left, uint32_t* right, float* nbox) {
    using Scan = rocprim::block_scan<uint32_t, kPlocTail>;
    __shared__ typename Scan::storage_type scan_storage;
    __shared__ float sb[6][kPlocTail];
    __shared__ uint32_t sid[kPlocTail], snn[kPlocTail];
    const uint32_t t = threadIdx.x;
    uint32_t n = words[W_PCOUNT + parity], made = words[W_PNODES + parity], iters = words[W_PITERS];
    if (n > (uint32_t)kPlocTail || n > cap) { if (t == 0u) words[W_PFAIL] = 1u; return; }
    if (t < n) {
        for (int k = 0; k < 6; ++k) sb[k][t] = cbox[(size_t)k * cap + t];
        sid[t] = cid[t];
    }
    __syncthreads();
    bool fail = false;
    while (n > 1u) {
        if (iters >= max_iters) { fail = true; break; }
        PlocBox me;
        uint32_t best = kPlocNone;
        if (t < n) {
            for (int k = 0; k < 3; ++k) { me.lo[k] = sb[k][t]; me.hi[k] = sb[3 + k][t]; }
            const uint32_t j0 = t > (uint32_t)kPlocRadius ? t - (uint32_t)kPlocRadius : 0u, j1 = min(n - 1u, t + (uint32_t)kPlocRadius);
            float bd = 0.0f;
            for (uint32_t j = j0; j <= j1; ++j) {
                if (j == t) continue;
                PlocBox o;
                for (int k = 0; k < 3; ++k) { o.lo[k] = sb[k][j]; o.hi[k] = sb[3 + k][j]; }
                const float d = ploc_distance(me, o);
                if (ploc_before(t, d, j, bd, best)) { best = j; bd = d; }
            }
            snn[t] = best;
        }
        __syncthreads();
        uint32_t merge = 0u, keep = 0u, id = 0u;
        if (t < n) {
            const bool mutual = best < n && snn[best] == t;
            merge = mutual && t < best ? 1u : 0u;
            keep = mutual && t > best ? 0u : 1u;
            id = sid[t];
        }
        uint32_t partner = 0u;
        if (merge) {
            PlocBox o;
            for (int k = 0; k < 3; ++k) { o.lo[k] = sb[k][best]; o.hi[k] = sb[3 + k][best]; }
            me = ploc_union(me, o);
            partner = sid[best];
        }
        uint32_t at = 0u, total = 0u;      // merges in the low half, kept clusters in the high half: n <= 1024 fits 16 bits each
        Scan().exclusive_scan(merge | (keep << 16), at, 0u, total, scan_storage);
        __syncthreads();                   // every read of the old array is done
        if (keep) {
            const uint32_t dest = at >> 16, node = made + (at & 0xFFFFu);
            if (merge && node < inner) {
                left[node] = id; right[node] = partner;
                for (int k = 0; k < 3; ++k) { nbox[(size_t)node * 6u + k] = me.lo[k]; nbox[(size_t)node * 6u + 3u + k] = me.hi[k]; }
                id = node;
            }
            for (int k = 0; k < 3; ++k) { sb[k][dest] = me.lo[k]; sb[3 + k][dest] = me.hi[k]; }
            sid[dest] = id;
        }
        made += total & 0xFFFFu; n = total >> 16; ++iters;
        __syncthreads();
    }
    if (t == 0u) { words[W_PITERS] = iters; words[W_PFAIL] = fail ? 1u : 0u; words[W_PNODES + parity] = made; words[W_PCOUNT + parity] = n; }
}

static inline dim3 ploc_grid(uint32_t n) { return dim3((n + kPlocBlock - 1) / kPlocBlock); }
static inline size_t ploc_align(size_t n) { return (n + 255u) & ~(size_t)255u; }

#define PLOC_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

hipError_t ploc_reserve(RebuildScratch& s, uint32_t num_tris) {
    PlocScratch& p = s.ploc;
    const uint32_t leaves = (num_tris + 1u) / 2u;
    if (p.base && p.cap >= leaves) return hipSuccess;
    if (p.base) (void)hipFree(p.base);
    p = PlocScratch{};
    PLOC_TRY(rocprim::exclusive_scan(nullptr, p.scan_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)leaves, rocprim::plus<unsigned long long>(), (hipStream_t) nullptr));
    const size_t box = ploc_align((size_t)leaves * 24u), word = ploc_align((size_t)leaves * 4u), wide = ploc_align((size_t)leaves * 8u);
    const size_t total = 3u * box + 3u * word + 2u * wide + ploc_align(p.scan_bytes);
    PLOC_TRY(hipMalloc(&p.base, total));
    uint8_t* q = (uint8_t*)p.base;
    auto take = [&](size_t n) { uint8_t* r = q; q += n; return r; };
    p.cbox[0] = (float*)take(box); p.cbox[1] = (float*)take(box); p.nbox = (float*)take(box);
    p.cid[0] = (uint32_t*)take(word); p.cid[1] = (uint32_t*)take(word); p.nn = (uint32_t*)take(word);
    p.flag = (unsigned long long*)take(wide); p.scan = (unsigned long long*)take(wide);
    p.scan_tmp = take(ploc_align(p.scan_bytes));
    p.bytes = total; p.cap = leaves;
    return hipSuccess;
}

hipError_t ploc_topology(RebuildScratch& s, const float4* tris, uint32_t num_tris, hipStream_t stream, uint32_t& iterations, bool& ok) {
    PlocScratch& p = s.ploc;
    iterations = 0; ok = false;
    const uint32_t leaves = (num_tris + 1u) / 2u;
    if (leaves < 2u || leaves > p.cap || leaves > s.cap_inner + 1u) return hipErrorInvalidValue;
    const uint32_t inner = leaves - 1u, cap = p.cap, max_iters = ploc_max_iterations(leaves);
    hipLaunchKernelGGL(ploc_leaf_kernel, ploc_grid(leaves), dim3(kPlocBlock), 0, stream, tris, num_tris, leaves, cap, p.cbox[0], p.cid[0], s.words);
    PLOC_TRY(hipGetLastError());
    // grids and the scan are sized by the last count the host has seen; the kernels read the live one
    uint32_t known = leaves, it = 0; int cur = 0;
    while (known > (uint32_t)kPlocTail) {
        if (it >= max_iters) { iterations = it; return hipSuccess; }
        for (int k = 0; k < kPlocChunk; ++k, ++it, cur ^= 1) {
            hipLaunchKernelGGL(ploc_nn_kernel, ploc_grid(known), dim3(kPlocBlock), 0, stream, p.cbox[cur], cap, s.words, it & 1u, p.nn);
            hipLaunchKernelGGL(ploc_flag_kernel, ploc_grid(known), dim3(kPlocBlock), 0, stream, p.nn, s.words, it & 1u, cap, known, p.flag);
            PLOC_TRY(hipGetLastError());
            size_t bytes = p.scan_bytes;
            PLOC_TRY(rocprim::exclusive_scan(p.scan_tmp, bytes, p.flag, p.scan, 0ull, (size_t)known, rocprim::plus<unsigned long long>(), stream));
            hipLaunchKernelGGL(ploc_merge_kernel, ploc_grid(known), dim3(kPlocBlock), 0, stream, p.cbox[cur], p.cid[cur], p.nn, p.flag, p.scan, cap, inner, s.words, it & 1u,
                               p.cbox[cur ^ 1], p.cid[cur ^ 1], s.left, s.right, p.nbox);
            PLOC_TRY(hipGetLastError());
        }
        PLOC_TRY(rebuild_fetch_words(s, stream));
        known = s.h_words[W_PCOUNT + (it & 1u)];
        if (known == 0u || known > leaves) return hipErrorUnknown;
    }
    hipLaunchKernelGGL(ploc_tail_kernel, dim3(1), dim3(kPlocTail), 0, stream, p.cbox[cur], p.cid[cur], cap, inner, s.words, it & 1u, max_iters, s.left, s.right, p.nbox);
    PLOC_TRY(hipGetLastError());
    PLOC_TRY(rebuild_fetch_words(s, stream));
    iterations = s.h_words[W_PITERS];
    ok = s.h_words[W_PFAIL] == 0u && s.h_words[W_PCOUNT + (it & 1u)] == 1u && s.h_words[W_PNODES + (it & 1u)] == inner;
    return hipSuccess;
}

} // namespace frt
