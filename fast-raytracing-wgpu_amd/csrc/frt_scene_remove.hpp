// frt_scene_remove.hpp — device side of frt_renderer_remove_materials / _meshes / _lights / _texture. Three kinds of kernel:
//   pool compaction, OUT OF PLACE: every surviving element of a pool (vertex positions, attributes, decoded normals, indices, mesh infos, material and
//     light records) goes to its new index in a buffer that is not part of the replica and enters it on the host afterwards;
//   record remap, IN PLACE: the id words of surviving records (material word of a shading record, mesh and material word of an instance record,
//     light_index and texture slots of a material) follow an old -> new table; every thread reads and writes its own word only;
//   history remap, IN PLACE: the material id every G-buffer set keeps per pixel (gpos.w) follows the same table.
// The host specification is SceneBuilder::remove_* (frt_scene.cpp), and the tables are made by its functions (removal_map, pack_mesh_removal).
#pragma once
#include "frt_scene.hpp"      // RemovedSpan, kGone
#include "frt_trace.hpp"
#include <hip/hip_runtime.h>

namespace frt {

// Elements removed in front of the element whose NEW index is g: `through` of the last span with new_begin <= g (spans sorted; several may share a
// new_begin, the last of them counts), 0 when there is none.
FRT_HD uint32_t removed_in_front(const RemovedSpan* spans, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;      // spans [0, lo) have new_begin <= g
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (spans[mid].new_begin <= g) lo = mid + 1u; else hi = mid; }
    return lo ? spans[lo - 1u].through : 0u;
}
// gpos.w of a pixel under an old -> new material table of `n` ids: a hit's id follows, a removed id (and any id the table does not hold) becomes
// kGoneMaterialWord, the miss word and everything else negative or not a number stays.
FRT_HD float remapped_material_word(float w, const uint32_t* map, uint32_t n) {
    if (!(w >= 0.0f)) return w;
    const uint32_t id = (uint32_t)(w + 0.1f);
    const uint32_t to = id < n ? map[id] : kGone;
    return to == kGone ? kGoneMaterialWord : (float)to;
}

// `count` surviving elements of `vecs` float4 each from `src` to `dst` (count * vecs work items; dst has room for them).
hipError_t launch_compact_vec4(const float4* src, float4* dst, uint32_t count, uint32_t vecs, const RemovedSpan* spans, uint32_t nspans, hipStream_t stream);
hipError_t launch_compact_u32(const uint32_t* src, uint32_t* dst, uint32_t count, const RemovedSpan* spans, uint32_t nspans, hipStream_t stream);
// The `count` surviving mesh infos with the offsets a scratch build gives them; the three tables hold one span per removed mesh, at the same index.
hipError_t launch_compact_mesh_infos(const MeshInfoView* src, MeshInfoView* dst, uint32_t count, const RemovedSpan* meshes, const RemovedSpan* verts, const RemovedSpan* indices,
                                     uint32_t nspans, hipStream_t stream);
// Word `word` of each of `count` records of `stride` words: an id below map_n with a surviving entry becomes that entry; anything else stays.
hipError_t launch_remap_words(uint32_t* records, uint32_t count, uint32_t stride, uint32_t word, const uint32_t* map, uint32_t map_n, hipStream_t stream);
// light_index and the five texture slots of `count` materials: `light_map` (or null) as above; slots above `color_layer` / `data_layer` (kGone: none) move down.
hipError_t launch_remap_materials(MaterialView* materials, uint32_t count, const uint32_t* light_map, uint32_t light_n, uint32_t color_layer, uint32_t data_layer, hipStream_t stream);
// gpos.w of `pixels` pixels of one G-buffer set.
hipError_t launch_remap_history(float4* gpos, uint32_t pixels, const uint32_t* map, uint32_t map_n, hipStream_t stream);

} // namespace frt
