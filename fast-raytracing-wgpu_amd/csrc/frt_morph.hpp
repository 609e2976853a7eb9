// frt_morph.hpp — morph targets ("Morph targets"): the arithmetic of SceneBuilder::set_mesh_morph_weights, __host__ __device__ so that the
// host specification (frt_scene.cpp) and the device pass (frt_pose_batch.hip) compile the same expressions: f32, no contraction, no fma written by hand. A header
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

// The device pass is pose_batch_morph_kernel (frt_pose_batch.hip): one thread per vertex, one 16-byte load of the base, per target one 12-byte delta
// (consecutive lanes read consecutive deltas of one target) and the target's weight, morphed_position, one 16-byte store.

} // namespace frt
