// TEST INFRASTRUCTURE ONLY — not linked into libfrt.so.
// trace4<ANY = true> (csrc/frt_trace.hpp) on the host over a scene's quad tree, both loops (the plain walk and the voting walk), with the whole tree
// staged as the node copy or none, on a stack that is watched: the words behind the ray's stack are poisoned before every ray, and the highest word
// the walk wrote is reported. tests/test_anyhit_order.py compares occluded / unoccluded with the brute-force loop over all triangles and the stack
// depth with what the builder states for the tree.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include "../../fast-raytracing-wgpu_amd/csrc/frt_mono.hpp"
#include <algorithm>
#include <vector>

using namespace frt;

extern "C" {
uint32_t ah_quad_nodes(const frt_scene* s) { return (uint32_t)s->b.quad_nodes.size(); }
uint32_t ah_stack_need(const frt_scene* s) { return s->b.quad_stack_need; }

// vote: 0 the plain walk, 1 the voting walk; cached: 1 = the walk reads its nodes from a staged copy of the tree. occluded_out[i] = 1 when ray i hits
// anything. Returns the deepest stack any ray reached, in entries.
uint32_t ah_trace_any(const frt_scene* s, int vote, int cached, uint32_t n, const float* o, const float* d, float tmin, const float* tmax, uint8_t* occluded_out) {
    const SceneBuilder& b = s->b;
    SceneView sv{};
    sv.nodes4 = reinterpret_cast<const float4*>(b.quad_nodes.data());
    sv.num_nodes4 = (uint32_t)b.quad_nodes.size();
    sv.tris = reinterpret_cast<const float4*>(b.tri_slots.data());
    sv.instances = reinterpret_cast<const InstanceView*>(b.instances_dev.data());
    std::vector<float4> copy(sv.nodes4, sv.nodes4 + (size_t)sv.num_nodes4 * 8u);
    const uint32_t* top = cached ? reinterpret_cast<const uint32_t*>(copy.data()) : nullptr;
    const uint32_t cache_n = cached ? sv.num_nodes4 : (uint32_t)kLdsTopNodes;
    const uint32_t kPoison = 0x7FFFFFFEu;      // neither a node index, nor a leaf reference (bit 31), nor "done"
    const uint32_t kWatched = 2u * (uint32_t)kStackDepth;
    std::vector<uint32_t> stack(kWatched);
    uint32_t deepest = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        std::fill(stack.begin(), stack.end(), kPoison);
        HitRec h;
        const f3 oo = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        if (vote) trace4<true, true>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h, top, cache_n);
        else trace4<true, false>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h, top, cache_n);
        occluded_out[i] = h.tri != 0xFFFFFFFFu;
        for (uint32_t k = kWatched; k-- > deepest;) if (stack[k] != kPoison) { deepest = k + 1u; break; }
    }
    return deepest;
}
}
