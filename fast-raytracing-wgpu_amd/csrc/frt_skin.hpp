// frt_skin.hpp — linear-blend skinning ("Skinning"): the arithmetic of SceneBuilder::set_mesh_pose, __host__ __device__ so that the host
// specification (frt_scene.cpp) and the device pass (frt_pose_batch.hip) compile the same expressions: f32, no contraction, no fma written by hand. A header of
// its own, beside frt_vertex_normal.hpp, because none of this is code of the frame's kernels.
#pragma once
#include "frt_math.hpp"

namespace frt {

// One skinned vertex. `p`: the bind position (x, y, z, w); `m[k]`: the column-major 4x4 of the joint in slot k (the layout of an instance transform; row 3 is
// not read); `w[k]`: the weight of slot k. Per slot and row r the point is world_triangle's expression (frt_scene.cpp), operation for operation:
//   q_k[r] = ((m[k][r] * x + m[k][4 + r] * y) + m[k][8 + r] * z) + m[k][12 + r]
// and the four slots blend in this order:
//   out[r] = ((w0 * q_0[r] + w1 * q_1[r]) + w2 * q_2[r]) + w3 * q_3[r]
// All four terms are evaluated, a weight of 0 included; the weights are used as given, not renormalised; out[3] is the bind pose's w.
FRT_HD void skinned_position(const float p[4], const float m[4][16], const float w[4], float out[4]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = ((m[k][r] * p[0] + m[k][4 + r] * p[1]) + m[k][8 + r] * p[2]) + m[k][12 + r];
        out[r] = ((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2]) + w[3] * q[3];
    }
    out[3] = p[3];
}

// The device pass is pose_batch_skin_kernel (frt_pose_batch.hip): one thread per vertex, one 16-byte load each of the bind position and the weights, one
// 8-byte load of the joints, four 16-byte columns of each of the four joints, skinned_position, one 16-byte store.

} // namespace frt
