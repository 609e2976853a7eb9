// TEST INFRASTRUCTURE ONLY — not linked into libfrt.so.
// trace4 (csrc/frt_trace.hpp) on the host over a scene's quad tree, closest-hit and any-hit, the plain and the voting loop, with the whole hit record
// handed back: tests/test_leaf_fetch.py compares it with the brute-force loop over all triangles on trees whose leaves meet each case of the leaf
// step's two in-line fetches (a single triangle in the array's only / last slot, a pair, three and four triangles).
// The triangle array handed to the walk is an exact-size copy on the heap, so that a read behind its last slot is a read behind an allocation.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include "../../fast-raytracing-wgpu_amd/csrc/frt_mono.hpp"
#include <cstring>
#include <vector>

using namespace frt;

extern "C" {
// out: 6 words per ray — t, u, v (float bits), triangle, instance, front. An any-hit ray reports triangle != miss only (the other words are zeroed).
void lf_trace(const frt_scene* s, int any, int vote, uint32_t n, const float* o, const float* d, float tmin, const float* tmax, uint32_t* out) {
    const SceneBuilder& b = s->b;
    SceneView sv{};
    sv.nodes4 = reinterpret_cast<const float4*>(b.quad_nodes.data());
    sv.num_nodes4 = (uint32_t)b.quad_nodes.size();
    const size_t tri_bytes = b.tri_slots.size() * sizeof(b.tri_slots[0]);
    float4* tris = static_cast<float4*>(::operator new(tri_bytes));
    std::memcpy(tris, b.tri_slots.data(), tri_bytes);
    sv.tris = tris;
    sv.instances = reinterpret_cast<const InstanceView*>(b.instances_dev.data());
    std::vector<uint32_t> stack((size_t)kStackDepth);
    for (uint32_t i = 0; i < n; ++i) {
        HitRec h;
        const f3 oo = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        if (any) { if (vote) trace4<true, true>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h); else trace4<true, false>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h); }
        else     { if (vote) trace4<false, true>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h); else trace4<false, false>(sv, oo, dd, tmin, tmax[i], stack.data(), 1u, h); }
        uint32_t* w = out + 6u * i;
        if (any) { w[0] = w[1] = w[2] = w[4] = w[5] = 0u; w[3] = h.tri; continue; }
        std::memcpy(w + 0, &h.t, 4); std::memcpy(w + 1, &h.u, 4); std::memcpy(w + 2, &h.v, 4);
        w[3] = h.tri; w[4] = h.inst; w[5] = h.front ? 1u : 0u;
    }
    ::operator delete(tris);
}
}
