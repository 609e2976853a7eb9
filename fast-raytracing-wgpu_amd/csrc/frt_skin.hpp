// frt_skin.hpp — linear-blend skinning ("Skinning"): the arithmetic of SceneBuilder::set_mesh_pose, __host__ __device__ so that the host
// specification (frt_scene.cpp) and the device pass (frt_skin.hip) compile the same expressions: f32, no contraction, no fma written by hand. A header of
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

// The device pass, in front of the device-input route of frt_deform.hpp (whose DeformInput::pos is `out`). One thread per vertex, consecutive threads on
// consecutive vertices: one 16-byte load each of the bind position and the weights, one 8-byte load of the joints, four 16-byte columns of each of the four
// joints, skinned_position, one 16-byte store. No LDS, nothing passed between the blocks. A joint index that is not below `njoints` (the bind call lets
// none in) raises the reject flag instead of being followed, and no thread stores past `out_len`. With `check_palette` (the palette is the caller's device
// memory, which the host has not seen) the first 4 * njoints threads also test one float4 of the palette each and raise the flag for a non-finite float,
// so that a bad joint no vertex names rejects the call as the host form refuses it.
struct SkinArgs {
    const float4* bind;          // [nverts] bind positions, xyzw
    const float4* weights;       // [nverts]
    const uint2* joints;         // [nverts] four uint16 each
    const float4* palette;       // [4 * njoints] columns
    float4* out;                 // [out_len] the skinned positions of this call
    uint32_t nverts, njoints, out_len;
    uint32_t check_palette;
    uint32_t* reject;            // DeformInput::reject: [0] is zeroed on the stream in front of this launch
};
hipError_t launch_mesh_skin(const SkinArgs& a, hipStream_t stream);

} // namespace frt
