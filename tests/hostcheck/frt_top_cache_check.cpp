// TEST INFRASTRUCTURE ONLY — not linked into libfrt.so.
// trace4 (csrc/frt_trace.hpp) on the host over a scene's quad tree WITH a copy of the tree's top, as the frame kernels keep one in LDS: the first
// min(cache_n, quad nodes) nodes staged into a separate array, and `cache_n` handed to the walk as its
// node-cache size. On the host a wave is one lane, so both forms of the wave-uniform test (leading steps only — the VOTE walk; any step — the plain
// walk) run exactly the code the kernels run. tests/test_lds_top_cache.py compares the hits with the brute-force loop over all triangles.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include "../../fast-raytracing-wgpu_amd/csrc/frt_mono.hpp"
#include <algorithm>
#include <vector>

using namespace frt;

extern "C" {
uint32_t tc_quad_nodes(const frt_scene* s) { return (uint32_t)s->b.quad_nodes.size(); }

// vote: 0 the plain walk (re-entrant test of the cache), 1 the voting walk (leading steps only). Returns the number of nodes staged.
uint32_t tc_trace(const frt_scene* s, int any, int vote, uint32_t cache_n, uint32_t n, const float* o, const float* d, float tmin, float tmax,
                  float* t_out, uint32_t* tri_out, float* uv_out, uint8_t* front_out) {
    const SceneBuilder& b = s->b;
    SceneView sv{};
    sv.nodes4 = reinterpret_cast<const float4*>(b.quad_nodes.data());
    sv.num_nodes4 = (uint32_t)b.quad_nodes.size();
    sv.tris = reinterpret_cast<const float4*>(b.tri_slots.data());
    sv.instances = reinterpret_cast<const InstanceView*>(b.instances_dev.data());
    const uint32_t staged = std::min(cache_n, sv.num_nodes4);
    // (poison behind the staged nodes: a walk that reads the copy past its end finds no box of the scene there)
    std::vector<float4> copy((size_t)std::max(staged, 1u) * 8u + 64u, make_float4(3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f));
    for (uint32_t i = 0; i < staged * 8u; ++i) copy[i] = sv.nodes4[i];
    const uint32_t* top = staged ? reinterpret_cast<const uint32_t*>(copy.data()) : nullptr;
    uint32_t stack[kStackDepth];
    for (uint32_t i = 0; i < n; ++i) {
        HitRec h;
        const f3 oo = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        if (any) { if (vote) trace4<true, true>(sv, oo, dd, tmin, tmax, stack, 1u, h, top, cache_n); else trace4<true, false>(sv, oo, dd, tmin, tmax, stack, 1u, h, top, cache_n); }
        else { if (vote) trace4<false, true>(sv, oo, dd, tmin, tmax, stack, 1u, h, top, cache_n); else trace4<false, false>(sv, oo, dd, tmin, tmax, stack, 1u, h, top, cache_n); }
        t_out[i] = h.tri != 0xFFFFFFFFu ? h.t : -1.0f;
        tri_out[i] = h.tri;
        uv_out[2 * i] = h.u; uv_out[2 * i + 1] = h.v;
        front_out[i] = h.front;
    }
    return staged;
}
}
