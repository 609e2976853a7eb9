// frt_refit.hip — kernels of frt_renderer_set_instance_transforms (frt_refit.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math): every f32 operation here is the one the host reference performs, in
// the same order, and no fma is written by hand. Box unions are min / max, which are exact: the level order of the device gives the host's boxes.
// Visibility between the steps comes from kernel boundaries on one stream (per-XCD L2s are not coherent within a kernel): no flags, no fences.
#include "frt_refit.hpp"

namespace frt {

static const int kRefitBlock = 256;
static const uint32_t kRefitLeaf = 0x80000000u, kRefitNone = 0xFFFFFFFFu;

// Threads [0, work): one triangle of a moved instance each, written into its slot (same id and instance bits). Threads [0, nrec): the moved
// instances' device records and registered lights.
__global__ void __launch_bounds__(kRefitBlock) instance_transform_kernel(SceneView sc, RefitArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kRefitBlock + threadIdx.x;
    if (g < a.nrec) {
        const MovedInstance& r = a.rec[g];
        const_cast<InstanceView*>(sc.instances)[r.id] = r.dev;
        if (r.light != kRefitNone && r.light < sc.num_lights) const_cast<LightView*>(sc.lights)[r.light] = r.light_rec;
    }
    if (g >= a.work) return;
    uint32_t lo = 0, hi = a.nrec;      // the last record with work_begin <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.rec[mid].work_begin <= g) lo = mid; else hi = mid; }
    const MovedInstance& r = a.rec[lo];
    const uint32_t j = g - r.work_begin;
    if (j >= r.tri_count) return;
    float4 p[3];
    float w[3][3];
    for (int k = 0; k < 3; ++k) p[k] = a.pos[r.pos_offset + sc.indices[r.index_offset + 3u * j + (uint32_t)k]];
    instance_world_vertices(r.m, p, w);
    const uint32_t id = r.first_tri + j, slot = a.slot_of[id];
    if (slot >= sc.num_tris) return;
    store_tri_slot(const_cast<float4*>(sc.tris) + (size_t)slot * 3u, w, id, r.id);
}

// max |coordinate| over the bounds of every triangle slot (v0, v0 + e1, v0 + e2): build_bvh2's `ext`. Non-negative f32 bits order as unsigned.
__global__ void __launch_bounds__(kRefitBlock) scene_extent_kernel(SceneView sc, unsigned int* ext) {
    __shared__ float part[kRefitBlock];
    const uint32_t s = blockIdx.x * (uint32_t)kRefitBlock + threadIdx.x;
    float e = 0.0f;
    if (s < sc.num_tris) {
        const float4 v0 = sc.tris[3u * s], e1 = sc.tris[3u * s + 1u], e2 = sc.tris[3u * s + 2u];
        const float v[9] = {v0.x, v0.y, v0.z, v0.x + e1.x, v0.y + e1.y, v0.z + e1.z, v0.x + e2.x, v0.y + e2.y, v0.z + e2.z};
        for (int k = 0; k < 9; ++k) e = fmaxf(e, fabsf(v[k]));
    }
    part[threadIdx.x] = e;
    __syncthreads();
    for (int w = kRefitBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] = fmaxf(part[threadIdx.x], part[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(ext, __float_as_uint(part[0]));
}

hipError_t launch_instance_transform(const SceneView& sc, const RefitArgs& a, hipStream_t stream) {
    const uint32_t n = a.work > a.nrec ? a.work : a.nrec;
    if (n > 0) hipLaunchKernelGGL(instance_transform_kernel, dim3((n + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, stream, sc, a);
    return launch_scene_extent(sc, a.ext, stream);
}

hipError_t launch_scene_extent(const SceneView& sc, unsigned int* ext, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ext, 0, sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    if (sc.num_tris > 0) hipLaunchKernelGGL(scene_extent_kernel, dim3((sc.num_tris + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, stream, sc, ext);
    return hipGetLastError();
}

// The padded box of a leaf reference (kLeafFlag | count << 24 | first slot), as SceneBuilder::refit computes it.
__device__ inline void leaf_box(const SceneView& sc, uint32_t ref, float pad, float lo[3], float hi[3]) {
    const uint32_t first = ref & 0xFFFFFFu, count = (ref >> 24) & 0x7Fu;
    for (int c = 0; c < 3; ++c) { lo[c] = __int_as_float(0x7F800000); hi[c] = -lo[c]; }
    for (uint32_t s = first; s < first + count && s < sc.num_tris; ++s) {
        const float4 v0 = sc.tris[3u * s], e1 = sc.tris[3u * s + 1u], e2 = sc.tris[3u * s + 2u];
        const float x[3] = {v0.x, v0.y, v0.z}, a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
        for (int c = 0; c < 3; ++c) {
            const float v1 = x[c] + a[c], v2 = x[c] + b[c];
            lo[c] = fminf(lo[c], fminf(x[c], fminf(v1, v2)));
            hi[c] = fmaxf(hi[c], fmaxf(x[c], fmaxf(v1, v2)));
        }
    }
    for (int c = 0; c < 3; ++c) { lo[c] = lo[c] - pad; hi[c] = hi[c] + pad; }
}

__global__ void __launch_bounds__(kRefitBlock) refit_level_kernel(SceneView sc, const unsigned int* ext, uint32_t p0, uint32_t p1, uint32_t q0, uint32_t q1) {
    const uint32_t g = blockIdx.x * (uint32_t)kRefitBlock + threadIdx.x;
    const float pad = 1e-4f * fmaxf(__uint_as_float(*ext), 1.0f);      // build_bvh2: 1e-4 * max(ext, 1)
    const uint32_t np = p1 - p0;
    if (g < np) {
        const uint32_t i = p0 + g;
        if (i >= sc.num_nodes) return;
        float4* n = const_cast<float4*>(sc.nodes) + (size_t)i * 4u;
        float4 ax[3] = {n[0], n[1], n[2]};
        const float4 refs = n[3];
        const uint32_t ref[2] = {__float_as_uint(refs.x), __float_as_uint(refs.y)};
        for (int c = 0; c < 2; ++c) {
            if (ref[c] == kRefitNone) continue;
            float lo[3], hi[3];
            if (ref[c] & kRefitLeaf) leaf_box(sc, ref[c], pad, lo, hi);
            else {
                if (ref[c] >= sc.num_nodes) continue;
                const float4* k = sc.nodes + (size_t)ref[c] * 4u;
                for (int a = 0; a < 3; ++a) { const float4 q = k[a]; lo[a] = fminf(q.x, q.y); hi[a] = fmaxf(q.z, q.w); }
            }
            for (int a = 0; a < 3; ++a) {
                if (c == 0) { ax[a].x = lo[a]; ax[a].z = hi[a]; } else { ax[a].y = lo[a]; ax[a].w = hi[a]; }
            }
        }
        n[0] = ax[0]; n[1] = ax[1]; n[2] = ax[2];
        return;
    }
    const uint32_t i = q0 + (g - np);
    if (i >= q1 || i >= sc.num_nodes4) return;
    // quad node: lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.z[4], hi.z[4], reference[4], unused[4]
    float* n = reinterpret_cast<float*>(const_cast<float4*>(sc.nodes4) + (size_t)i * 8u);
    float box[24];
    uint32_t ref[4];
    for (int k = 0; k < 6; ++k) { const float4 v = reinterpret_cast<const float4*>(n)[k]; box[4 * k] = v.x; box[4 * k + 1] = v.y; box[4 * k + 2] = v.z; box[4 * k + 3] = v.w; }
    { const float4 v = reinterpret_cast<const float4*>(n)[6]; ref[0] = __float_as_uint(v.x); ref[1] = __float_as_uint(v.y); ref[2] = __float_as_uint(v.z); ref[3] = __float_as_uint(v.w); }
    for (int c = 0; c < 4; ++c) {
        if (ref[c] == kRefitNone) continue;
        float lo[3], hi[3];
        if (ref[c] & kRefitLeaf) leaf_box(sc, ref[c], pad, lo, hi);
        else {
            if (ref[c] >= sc.num_nodes4) continue;
            const float4* k = sc.nodes4 + (size_t)ref[c] * 8u;
            const float4 kr = k[6];
            const uint32_t kref[4] = {__float_as_uint(kr.x), __float_as_uint(kr.y), __float_as_uint(kr.z), __float_as_uint(kr.w)};
            for (int a = 0; a < 3; ++a) {
                const float4 l = k[2 * a], h = k[2 * a + 1];
                const float ls[4] = {l.x, l.y, l.z, l.w}, hs[4] = {h.x, h.y, h.z, h.w};
                lo[a] = __int_as_float(0x7F800000); hi[a] = -lo[a];
                for (int j = 0; j < 4; ++j) if (kref[j] != kRefitNone) { lo[a] = fminf(lo[a], ls[j]); hi[a] = fmaxf(hi[a], hs[j]); }
            }
        }
        for (int a = 0; a < 3; ++a) { box[8 * a + c] = lo[a]; box[8 * a + 4 + c] = hi[a]; }
    }
    for (int k = 0; k < 6; ++k) reinterpret_cast<float4*>(n)[k] = make_float4(box[4 * k], box[4 * k + 1], box[4 * k + 2], box[4 * k + 3]);
}

hipError_t launch_refit_level(const SceneView& sc, const unsigned int* ext, uint32_t p0, uint32_t p1, uint32_t q0, uint32_t q1, hipStream_t stream) {
    const uint32_t n = (p1 - p0) + (q1 - q0);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_level_kernel, dim3((n + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, stream, sc, ext, p0, p1, q0, q1);
    return hipGetLastError();
}

} // namespace frt
