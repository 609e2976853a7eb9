// frt_mesh_edit.hip — the kernel of frt_renderer_add_meshes (frt_mesh_edit.hpp).
// Built with the library's contract flags (-ffp-contract=off, no fast math, IEEE division and square root): the only arithmetic is
// decode_octahedral_normal, the function the host build decodes a vertex normal with, so the decoded normals equal the host's bit for bit.
// Every thread reads staged data of this call and writes pool elements that no other thread of the launch writes and none reads: plain vector loads
// and stores, consecutive threads on consecutive elements, no LDS, no atomics. The kernels that read the pools (frt_renderer_add_instances, the
// deformation, the instance update) are later launches on the same stream: the kernel boundary is all the visibility they need. Every thread checks
// its destination against the pool's capacity before it stores.
#include "frt_mesh_edit.hpp"
#include "frt_shade.hpp"

namespace frt {

static const int kMeshEditBlock = 256;      // four waves of 64

// The last record whose `begin` (vert_begin or index_begin, ascending) is <= g.
template <class Begin>
__device__ inline uint32_t mesh_of(const MeshAppend* rec, uint32_t n, uint32_t g, Begin begin) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (begin(rec[mid]) <= g) lo = mid; else hi = mid; }
    return lo;
}

// Threads [0, nverts): one new vertex each — position, attribute record and decoded normal. Threads [nverts, nverts + nidx): one index each.
// Threads [0, nrec): the mesh-info records.
__global__ void __launch_bounds__(kMeshEditBlock) mesh_append_kernel(MeshAppendArgs a) {
    const uint32_t g = blockIdx.x * (uint32_t)kMeshEditBlock + threadIdx.x;
    if (g < a.nrec) {
        const MeshAppend r = a.rec[g];
        if (a.mesh_base + g < a.cap_meshes) a.out_infos[a.mesh_base + g] = MeshInfoView{r.vert_base, r.index_base, 0u, 0u};
    }
    if (g < a.nverts) {
        const MeshAppend r = a.rec[mesh_of(a.rec, a.nrec, g, [](const MeshAppend& m) { return m.vert_begin; })];
        const uint32_t j = g - r.vert_begin;
        if (j >= r.nverts) return;
        const uint32_t dst = r.vert_base + j;
        if (dst >= a.cap_verts) return;
        const float4 nu = a.attrs[2u * (size_t)g], tg = a.attrs[2u * (size_t)g + 1u];
        a.out_pos[dst] = a.pos[g];
        a.out_attrs[2u * (size_t)dst] = nu;
        a.out_attrs[2u * (size_t)dst + 1u] = tg;
        const f3 n = decode_octahedral_normal(nu.x, nu.y);
        a.out_normals[dst] = make_float4(n.x, n.y, n.z, 0.0f);
        return;
    }
    const uint32_t h = g - a.nverts;
    if (h >= a.nidx) return;
    const MeshAppend r = a.rec[mesh_of(a.rec, a.nrec, h, [](const MeshAppend& m) { return m.index_begin; })];
    const uint32_t j = h - r.index_begin;
    if (j >= r.nidx) return;
    const uint32_t dst = r.index_base + j;
    if (dst >= a.cap_indices) return;
    a.out_idx[dst] = a.idx[h];
}

hipError_t launch_mesh_append(const MeshAppendArgs& a, hipStream_t stream) {
    const uint64_t work = (uint64_t)a.nverts + a.nidx;
    if (a.nrec == 0 || work == 0) return hipSuccess;
    if (work > 0xFFFFFF00ull) return hipErrorInvalidValue;      // (the work-item index is 32 bits; frt_renderer_add_meshes checks it first)
    hipLaunchKernelGGL(mesh_append_kernel, dim3((uint32_t)((work + kMeshEditBlock - 1) / kMeshEditBlock)), dim3(kMeshEditBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace frt
