// frt_scene_remove.hip — the kernels of frt_renderer_remove_materials / _meshes / _lights / _texture (frt_scene_remove.hpp).
// Built with the library's contract flags; the only arithmetic on a float is the history word's (id = (uint32_t)(w + 0.1f), back through (float)), which
// is exact for every id below 2^24. Plain vector loads and stores, consecutive threads on consecutive elements, no LDS, no atomics. A compaction reads
// the replica's pool and writes a buffer nothing else reads until the host has put it into the replica; a remap reads and writes one word per thread and
// no thread reads another's. The kernels that read the results are later launches on the same stream: the kernel boundary is the visibility they need.
// Every launch covers exactly the elements the host counted; each thread checks its index against that count before it touches memory.
#include "frt_scene_remove.hpp"

namespace frt {

static const int kRemoveBlock = 256;      // four waves of 64
static dim3 blocks_for(uint64_t work) { return dim3((uint32_t)((work + kRemoveBlock - 1) / kRemoveBlock)); }

__global__ void __launch_bounds__(kRemoveBlock) compact_vec4_kernel(const float4* src, float4* dst, uint32_t work, uint32_t vecs, const RemovedSpan* spans, uint32_t nspans) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= work) return;
    const uint32_t e = g / vecs, v = g - e * vecs;
    const size_t old = (size_t)e + removed_in_front(spans, nspans, e);
    dst[g] = src[old * vecs + v];
}
__global__ void __launch_bounds__(kRemoveBlock) compact_u32_kernel(const uint32_t* src, uint32_t* dst, uint32_t count, const RemovedSpan* spans, uint32_t nspans) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= count) return;
    dst[g] = src[(size_t)g + removed_in_front(spans, nspans, g)];
}
__global__ void __launch_bounds__(kRemoveBlock) compact_mesh_infos_kernel(const MeshInfoView* src, MeshInfoView* dst, uint32_t count, const RemovedSpan* meshes, const RemovedSpan* verts,
                                                                          const RemovedSpan* indices, uint32_t nspans) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= count) return;
    const uint32_t k = removed_in_front(meshes, nspans, g);      // removed meshes in front of this one = spans of the other tables in front of its elements
    const MeshInfoView m = src[(size_t)g + k];
    const uint32_t vgone = k ? verts[k - 1u].through : 0u, igone = k ? indices[k - 1u].through : 0u;
    dst[g] = MeshInfoView{m.vertex_offset - vgone, m.index_offset - igone, 0u, 0u};
}
__global__ void __launch_bounds__(kRemoveBlock) remap_words_kernel(uint32_t* records, uint32_t count, uint32_t stride, uint32_t word, const uint32_t* map, uint32_t map_n) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= count) return;
    uint32_t* p = records + (size_t)g * stride + word;
    const uint32_t id = *p;
    if (id >= map_n) return;
    const uint32_t to = map[id];
    if (to != kGone && to != id) *p = to;
}
__device__ inline uint32_t slot_without(uint32_t slot, uint32_t layer) { return slot != 0xFFFFu && layer != kGone && slot > layer ? slot - 1u : slot; }
// One thread per word: light_index, tex_info_0, tex_info_1, tex_info_2 of material g / 4 (words 11 .. 14 of its 16).
__global__ void __launch_bounds__(kRemoveBlock) remap_material_words_kernel(uint32_t* materials, uint32_t count, const uint32_t* light_map, uint32_t light_n, uint32_t color_layer,
                                                                            uint32_t data_layer) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= 4u * count) return;
    const uint32_t which = g & 3u;
    uint32_t* p = materials + (size_t)(g >> 2) * 16u + 11u + which;
    const uint32_t w = *p;
    uint32_t to = w;
    if (which == 0u) { if (light_map && w < light_n && light_map[w] != kGone) to = light_map[w]; }      // (a negative index is >= 2^31: never below light_n)
    else if (which == 1u) to = slot_without(w & 0xFFFFu, color_layer) | (slot_without(w >> 16, data_layer) << 16);
    else if (which == 2u) to = slot_without(w & 0xFFFFu, data_layer) | (slot_without(w >> 16, color_layer) << 16);
    else to = slot_without(w & 0xFFFFu, data_layer) | (w & 0xFFFF0000u);
    if (to != w) *p = to;
}
__global__ void __launch_bounds__(kRemoveBlock) remap_history_kernel(float* gpos, uint32_t pixels, const uint32_t* map, uint32_t map_n) {
    const uint32_t g = blockIdx.x * (uint32_t)kRemoveBlock + threadIdx.x;
    if (g >= pixels) return;
    float* p = gpos + 4u * (size_t)g + 3u;
    const float w = *p, to = remapped_material_word(w, map, map_n);
    if (w >= 0.0f) *p = to;
}

hipError_t launch_compact_vec4(const float4* src, float4* dst, uint32_t count, uint32_t vecs, const RemovedSpan* spans, uint32_t nspans, hipStream_t stream) {
    const uint64_t work = (uint64_t)count * vecs;
    if (work == 0) return hipSuccess;
    if (work > 0xFFFFFF00ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_vec4_kernel, blocks_for(work), dim3(kRemoveBlock), 0, stream, src, dst, (uint32_t)work, vecs, spans, nspans);
    return hipGetLastError();
}
hipError_t launch_compact_u32(const uint32_t* src, uint32_t* dst, uint32_t count, const RemovedSpan* spans, uint32_t nspans, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (count > 0xFFFFFF00u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_u32_kernel, blocks_for(count), dim3(kRemoveBlock), 0, stream, src, dst, count, spans, nspans);
    return hipGetLastError();
}
hipError_t launch_compact_mesh_infos(const MeshInfoView* src, MeshInfoView* dst, uint32_t count, const RemovedSpan* meshes, const RemovedSpan* verts, const RemovedSpan* indices,
                                     uint32_t nspans, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(compact_mesh_infos_kernel, blocks_for(count), dim3(kRemoveBlock), 0, stream, src, dst, count, meshes, verts, indices, nspans);
    return hipGetLastError();
}
hipError_t launch_remap_words(uint32_t* records, uint32_t count, uint32_t stride, uint32_t word, const uint32_t* map, uint32_t map_n, hipStream_t stream) {
    if (count == 0 || map_n == 0) return hipSuccess;
    hipLaunchKernelGGL(remap_words_kernel, blocks_for(count), dim3(kRemoveBlock), 0, stream, records, count, stride, word, map, map_n);
    return hipGetLastError();
}
hipError_t launch_remap_materials(MaterialView* materials, uint32_t count, const uint32_t* light_map, uint32_t light_n, uint32_t color_layer, uint32_t data_layer, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(remap_material_words_kernel, blocks_for(4ull * count), dim3(kRemoveBlock), 0, stream, reinterpret_cast<uint32_t*>(materials), count, light_map, light_n,
                       color_layer, data_layer);
    return hipGetLastError();
}
hipError_t launch_remap_history(float4* gpos, uint32_t pixels, const uint32_t* map, uint32_t map_n, hipStream_t stream) {
    if (pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(remap_history_kernel, blocks_for(pixels), dim3(kRemoveBlock), 0, stream, reinterpret_cast<float*>(gpos), pixels, map, map_n);
    return hipGetLastError();
}

} // namespace frt
