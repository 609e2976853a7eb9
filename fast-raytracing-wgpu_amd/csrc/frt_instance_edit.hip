// frt_instance_edit.hip — kernels of frt_renderer_add_instances / _remove_instances (frt_instance_edit.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math); the only arithmetic is instance_world_vertices (frt_refit.hpp), the
// rest is a gather. Both kernels read the replica and write buffers that are NOT part of it: no thread reads what another thread of the launch
// writes, so there is nothing to order inside a launch (per-XCD L2s are not coherent within one); the extent pass and the rebuild that read the
// new buffers are later launches on the same stream. Every thread checks its index against the new counts before it stores.
#include "frt_instance_edit.hpp"

namespace frt {

static const int kEditBlock = 256;      // four waves of 64

// Threads [0, work): one triangle of an appended instance each — the whole slot (id and instance words included: no old slot exists), its entry of
// the id -> slot table (slot = id) and its whole shading record. Threads [0, nrec): the appended instances' device records.
__global__ void __launch_bounds__(kEditBlock) instances_append_kernel(SceneView sc, AppendArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kEditBlock + threadIdx.x;
    if (g < a.nrec) {
        const AppendInstance& r = a.rec[g];
        if (r.id < a.num_instances) a.out.instances[r.id] = r.dev;
    }
    if (g >= a.work) return;
    uint32_t lo = 0, hi = a.nrec;      // the last record with work_begin <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.rec[mid].work_begin <= g) lo = mid; else hi = mid; }
    const AppendInstance& r = a.rec[lo];
    const uint32_t j = g - r.work_begin;
    if (j >= r.tri_count) return;
    const uint32_t id = r.first_tri + j;
    if (id >= a.num_tris) return;
    uint32_t v[3];
    float4 p[3];
    float w[3][3];
    for (int k = 0; k < 3; ++k) { v[k] = sc.indices[r.index_offset + 3u * j + (uint32_t)k]; p[k] = a.pos[r.pos_offset + v[k]]; }
    instance_world_vertices(r.m, p, w);
    store_tri_slot(a.out.tris + (size_t)id * 3u, w, id, r.id);
    a.out.slot_of[id] = id;
    const float4* at = reinterpret_cast<const float4*>(sc.attributes + r.attr_offset);      // per vertex: (normal.xy, uv.xy) (tangent.xyzw)
    float4 n[3], nu[3], tg[3];
    for (int k = 0; k < 3; ++k) { n[k] = a.normals[r.attr_offset + v[k]]; nu[k] = at[2u * v[k]]; tg[k] = at[2u * v[k] + 1u]; }
    float4* rec = a.out.shade_tris + (size_t)id * 8u;
    store_shade_corners(rec, n, nu, tg);
    rec[6] = make_float4(tg[0].w, __uint_as_float(r.dev.mat_id), 0.0f, 0.0f);
    rec[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// How many removed ranges lie in front of position `g` of the new numbering (`key`: new_tri or new_inst of a range), by binary search: the ranges
// are sorted, and neighbours that were removed together share a position.
template <class Key>
__device__ inline uint32_t ranges_before(const RemovedRange* rng, uint32_t n, uint32_t g, Key key) {
    uint32_t lo = 0, hi = n;      // the first range with key > g
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (key(rng[mid]) <= g) lo = mid + 1u; else hi = mid; }
    return lo;
}

// Threads [0, num_tris): the surviving triangle with NEW id g. Its old id is g + the triangles removed in front of it; its slot and its shading
// record are copied under the new id (slot = id), its instance word less the instances removed in front of it. Threads [0, num_instances): the
// surviving instance records, compacted, first_tri less the triangles removed in front.
__global__ void __launch_bounds__(kEditBlock) instances_remove_kernel(SceneView sc, RemoveArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kEditBlock + threadIdx.x;
    if (g < a.num_instances) {
        const uint32_t k = ranges_before(a.rng, a.nrng, g, [](const RemovedRange& r) { return r.new_inst; });
        const uint32_t from = g + k;
        if (from < a.old_instances) {
            InstanceView in = sc.instances[from];
            in.first_tri -= k > 0u ? a.rng[k - 1u].tris_through : 0u;
            a.out.instances[g] = in;
        }
    }
    if (g >= a.num_tris) return;
    const uint32_t k = ranges_before(a.rng, a.nrng, g, [](const RemovedRange& r) { return r.new_tri; });
    const uint32_t old_id = g + (k > 0u ? a.rng[k - 1u].tris_through : 0u);
    if (old_id >= a.old_tris) return;
    const uint32_t slot = a.slot_of[old_id];
    if (slot >= a.old_tris) return;
    const float4* t = sc.tris + (size_t)slot * 3u;
    const float4 t0 = t[0], t1 = t[1], t2 = t[2];
    float4* o = a.out.tris + (size_t)g * 3u;
    o[0] = make_float4(t0.x, t0.y, t0.z, __uint_as_float(g));
    o[1] = make_float4(t1.x, t1.y, t1.z, __uint_as_float(__float_as_uint(t1.w) - k));
    o[2] = t2;
    a.out.slot_of[g] = g;
    const float4* from = sc.shade_tris + (size_t)old_id * 8u;
    float4* to = a.out.shade_tris + (size_t)g * 8u;
    for (int q = 0; q < 8; ++q) to[q] = from[q];
}

hipError_t launch_instances_append(const SceneView& sc, const AppendArgs& a, hipStream_t stream) {
    const uint32_t n = a.work > a.nrec ? a.work : a.nrec;
    if (a.nrec == 0 || n == 0) return hipSuccess;
    hipLaunchKernelGGL(instances_append_kernel, dim3((n + kEditBlock - 1) / kEditBlock), dim3(kEditBlock), 0, stream, sc, a);
    return hipGetLastError();
}

hipError_t launch_instances_remove(const SceneView& sc, const RemoveArgs& a, hipStream_t stream) {
    const uint32_t n = a.num_tris > a.num_instances ? a.num_tris : a.num_instances;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(instances_remove_kernel, dim3((n + kEditBlock - 1) / kEditBlock), dim3(kEditBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
