// frt_morph.hpp — morph targets ("Morph targets"): the arithmetic of SceneBuilder::set_mesh_morph_weights, __host__ __device__ so that the
// host specification (frt_scene.cpp) and the device pass (frt_morph.hip) compile the same expressions: f32, no contraction, no fma written by hand. A header
// of its own, beside frt_skin.hpp, because none of this is code of the frame's kernels.
#pragma once
#include "frt_math.hpp"
#include "../../include/frt.h"      // FRT_MAX_MORPH_TARGETS

namespace frt {

// One morphed vertex. `b`: the base position (x, y, z, w); `d`: the delta (dx, dy, dz) of target 0 for this vertex, the delta of target t `stride` floats
// further per t (the targets are stored target-major: stride = 3 * nverts); `w[t]`: the weight of target t. Per row r in 0..2, in target order:
//   out[r] = ((...((b[r] + w[0] * d_0[r]) + w[1] * d_1[r]) ...) + w[T - 1] * d_{T-1}[r])
// Every term is evaluated, a weight of 0 included; the weights are used as given (negative and above 1 too, not normalised); out[3] is the base's w.
// The loop is unrolled by four so that the device issues the loads of four targets in front of the adds that depend on one another; the order of the
// adds is the loop's.
FRT_HD void morphed_position(const float b[4], const float* d, size_t stride, const float* w, uint32_t ntargets, float out[4]) {
    float x = b[0], y = b[1], z = b[2];
#pragma unroll 4
    for (uint32_t t = 0; t < ntargets; ++t) {
        const float* q = d + (size_t)t * stride;
        const float wt = w[t];
        x = x + wt * q[0];
        y = y + wt * q[1];
        z = z + wt * q[2];
    }
    out[0] = x; out[1] = y; out[2] = z; out[3] = b[3];
}

// The device pass, in front of the device-input route of frt_deform.hpp (whose DeformInput::pos is `out`) or, in the combined call, of frt_skin.hpp's pass
// (whose SkinArgs::bind is `out`). One thread per vertex, consecutive threads on consecutive vertices: one 16-byte load of the base, per target one
// 12-byte delta (consecutive lanes read consecutive deltas of one target) and the target's weight, which is one address for the whole wave,
// morphed_position, one 16-byte store. No LDS, nothing passed between the blocks, and no thread stores past `out_len`. With `check_weights` (the weights
// are the caller's device memory, which the host has not seen) the first ntargets threads also test one weight each and raise the reject flag for a
// non-finite one, so that a bad weight whose target moves nothing rejects the call as the host form refuses it.
struct MorphArgs {
    const float4* base;          // [nverts] base positions, xyzw
    const float* deltas;         // [ntargets][nverts][3]
    const float* weights;        // [ntargets]
    float4* out;                 // [out_len] the morphed positions of this call
    uint32_t nverts, ntargets, out_len;
    uint32_t check_weights;
    uint32_t* reject;            // DeformInput::reject: [0] is zeroed on the stream in front of this launch
};
hipError_t launch_mesh_morph(const MorphArgs& a, hipStream_t stream);

} // namespace frt
