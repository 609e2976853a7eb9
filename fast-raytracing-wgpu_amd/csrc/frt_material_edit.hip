// frt_material_edit.hip — the kernel of frt_renderer_set_instance_materials (frt_material_edit.hpp).
// Every thread stores one 4-byte word that no other thread of the launch stores (the host passes each instance once, and instances own disjoint
// triangle ranges): plain stores, no read-modify-write of a record, no atomics. The frame kernels that read the words are later launches on the
// same stream (or ordered behind it), so the kernel boundary is all the visibility they need.
#include "frt_material_edit.hpp"

namespace frt {

static const int kMaterialEditBlock = 256;      // four waves of 64
static const uint32_t kShadeTriWords = 32u, kShadeTriMatWord = 25u;      // ShadeTri: 128 B, the material id in q[25]
static const uint32_t kInstanceWords = 16u, kInstanceMatWord = 1u;       // InstanceView: 64 B, mat_id its second word

// Threads [0, work): one triangle of an edited instance each. Threads [0, nrec): the edited instances' device records.
__global__ void __launch_bounds__(kMaterialEditBlock) instance_materials_kernel(SceneView sc, MaterialEditArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kMaterialEditBlock + threadIdx.x;
    if (g < a.nrec) {
        const MaterialEditInstance r = a.rec[g];
        if (r.id < a.num_instances)
            reinterpret_cast<uint32_t*>(const_cast<InstanceView*>(sc.instances))[(size_t)r.id * kInstanceWords + kInstanceMatWord] = r.mat_id;
    }
    if (g >= a.work) return;
    uint32_t lo = 0, hi = a.nrec;      // the last record with work_begin <= g: g < the next one's work_begin, so the triangle is this instance's
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.rec[mid].work_begin <= g) lo = mid; else hi = mid; }
    const MaterialEditInstance r = a.rec[lo];
    const uint32_t id = r.first_tri + (g - r.work_begin);
    if (id >= sc.num_tris) return;
    reinterpret_cast<uint32_t*>(const_cast<float4*>(sc.shade_tris))[(size_t)id * kShadeTriWords + kShadeTriMatWord] = r.mat_id;
}

hipError_t launch_instance_materials(const SceneView& sc, const MaterialEditArgs& a, hipStream_t stream) {
    const uint32_t n = a.work > a.nrec ? a.work : a.nrec;
    if (a.nrec == 0 || n == 0) return hipSuccess;
    hipLaunchKernelGGL(instance_materials_kernel, dim3((n + kMaterialEditBlock - 1) / kMaterialEditBlock), dim3(kMaterialEditBlock), 0, stream, sc, a);
    return hipGetLastError();
}

} // namespace frt
