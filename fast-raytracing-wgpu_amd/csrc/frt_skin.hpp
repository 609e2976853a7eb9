// frt_skin.hpp — skinning, the linear blend ("Skinning") and below it the dual-quaternion blend: the arithmetic of SceneBuilder::set_mesh_pose, __host__ __device__ so that the host
// specification (frt_scene.cpp) and the device pass (frt_pose_batch.hip) compile the same expressions: f32, no contraction, no fma written by hand. A header of
// its own, beside frt_vertex_normal.hpp, because none of this is code of the frame's kernels.
#pragma once
#include "../../include/frt.h"
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

// ---- dual-quaternion skinning ("Dual-quaternion skinning"; Kavan et al.): the arithmetic of a mesh bound with FRT_SKIN_DUAL_QUATERNION.
// The same rules: f32, no contraction, no fma written by hand, rsqrt_exact and sqrtf_ of frt_math.hpp, every product and sum once and in the order
// written here (include/frt.h spells it out). A joint is a rigid transform times ONE uniform scale: shear and non-uniform scale are not represented
// (the columns are normalised one by one and their lengths averaged), and a matrix that has them is skinned as the nearest thing this form can say.

// One joint: the uniform scale, the rotation's unit quaternion (x, y, z, w) and the dual part 0.5 (t, 0) qr.
struct SkinDualQuat { float s, r[4], d[4]; };

// The joint of the column-major 4x4 `m` (row 3 is not read). Per column c its squared length n_c = (m[4c]^2 + m[4c+1]^2) + m[4c+2]^2;
// s = ((sqrt n_0 + sqrt n_1) + sqrt n_2) * (1/3 rounded to f32); R's column c is m's times rsqrt_exact(n_c). With R_rc the entry of row r and column c
// and t = (R_00 + R_11) + R_22, the quaternion comes from the greatest of (t, R_00, R_11, R_22), the first of equals in that order (Shepperd), WITHOUT
// its square root and division, which the normalisation that follows anyway performs:
//   t:    (R_21 - R_12, R_02 - R_20, R_10 - R_01, 1 + t)                      = 4 w (x, y, z, w)
//   R_00: (((1 + R_00) - R_11) - R_22, R_01 + R_10, R_02 + R_20, R_21 - R_12) = 4 x (x, y, z, w)
//   R_11: (R_01 + R_10, ((1 + R_11) - R_00) - R_22, R_12 + R_21, R_02 - R_20) = 4 y (x, y, z, w)
//   R_22: (R_02 + R_20, R_12 + R_21, ((1 + R_22) - R_00) - R_11, R_10 - R_01) = 4 z (x, y, z, w)
// times rsqrt_exact(((x x + y y) + z z) + w w). The leading component of the branch taken is at least 1 before the normalisation, so nothing cancels;
// the sign of the result is the branch's (w may be negative), which the vertex's sigma takes care of. With t = (m[12], m[13], m[14]):
//   d.x = 0.5 ((tx rw + ty rz) - tz ry)   d.y = 0.5 ((ty rw + tz rx) - tx rz)   d.z = 0.5 ((tz rw + tx ry) - ty rx)   d.w = -0.5 ((tx rx + ty ry) + tz rz)
// A zero column: rsqrt_exact(0) is an infinity, the column NaN and the quaternion with it; a column whose squared length overflows: s is an infinity.
// Both reach every vertex that names the joint as a non-finite coordinate, which the overflow rule of set_mesh_pose refuses.
FRT_HD SkinDualQuat skin_dq_of_joint(const float m[16]) {
    const float n0 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2], n1 = (m[4] * m[4] + m[5] * m[5]) + m[6] * m[6], n2 = (m[8] * m[8] + m[9] * m[9]) + m[10] * m[10];
    const float i0 = rsqrt_exact(n0), i1 = rsqrt_exact(n1), i2 = rsqrt_exact(n2);
    SkinDualQuat j;
    j.s = ((sqrtf_(n0) + sqrtf_(n1)) + sqrtf_(n2)) * 0.333333343f;
    const float r00 = m[0] * i0, r10 = m[1] * i0, r20 = m[2] * i0, r01 = m[4] * i1, r11 = m[5] * i1, r21 = m[6] * i1, r02 = m[8] * i2, r12 = m[9] * i2, r22 = m[10] * i2;
    const float t = (r00 + r11) + r22;
    float x, y, z, w;
    if (t >= r00 && t >= r11 && t >= r22) { x = r21 - r12; y = r02 - r20; z = r10 - r01; w = 1.0f + t; }
    else if (r00 >= r11 && r00 >= r22) { x = ((1.0f + r00) - r11) - r22; y = r01 + r10; z = r02 + r20; w = r21 - r12; }
    else if (r11 >= r22) { x = r01 + r10; y = ((1.0f + r11) - r00) - r22; z = r12 + r21; w = r02 - r20; }
    else { x = r02 + r20; y = r12 + r21; z = ((1.0f + r22) - r00) - r11; w = r10 - r01; }
    const float inv = rsqrt_exact(((x * x + y * y) + z * z) + w * w);
    x = x * inv; y = y * inv; z = z * inv; w = w * inv;
    j.r[0] = x; j.r[1] = y; j.r[2] = z; j.r[3] = w;
    const float tx = m[12], ty = m[13], tz = m[14];
    j.d[0] = 0.5f * ((tx * w + ty * z) - tz * y);
    j.d[1] = 0.5f * ((ty * w + tz * x) - tx * z);
    j.d[2] = 0.5f * ((tz * w + tx * y) - ty * x);
    j.d[3] = -0.5f * ((tx * x + ty * y) + tz * z);
    return j;
}

// One vertex under the four joints of its slots. The pivot is the first slot of greatest weight; sigma_k = -1 where ((r_k.x r_p.x + r_k.y r_p.y) +
// r_k.z r_p.z) + r_k.w r_p.w < 0, else 1 (a dot product of exactly 0, and the pivot's own, give 1); per component c of the eight
//   b[c] = ((w0 (sigma_0 q_0[c]) + w1 (sigma_1 q_1[c])) + w2 (sigma_2 q_2[c])) + w3 (sigma_3 q_3[c])        (sigma q is a sign change: exact)
// and s_b the same sum of the scales without sigma. All four terms are evaluated, weights as given. Both halves of b times
// rsqrt_exact(((br.x^2 + br.y^2) + br.z^2) + br.w^2) give (r, d); with u = r.xyz, v = s_b * p.xyz (three products) and cross(a, b) =
// (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x):
//   rot = v + 2 cross(u, cross(u, v) + r.w v)            tr = 2 ((r.w d.xyz - d.w u) + cross(u, d.xyz))            out.xyz = rot + tr,  out.w = p.w
// A blend whose real part cancels to zero has an infinite rsqrt_exact and NaN coordinates: refused by the overflow rule, as above.
FRT_HD void skinned_position_dq(const float p[4], const SkinDualQuat j[4], const float w[4], float out[4]) {
    int pi = 0;
    float pw = w[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (w[k] > pw) { pi = k; pw = w[k]; }
    float pr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) pr[c] = pi == 0 ? j[0].r[c] : (pi == 1 ? j[1].r[c] : (pi == 2 ? j[2].r[c] : j[3].r[c]));
    float sg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sg[k] = (((j[k].r[0] * pr[0] + j[k].r[1] * pr[1]) + j[k].r[2] * pr[2]) + j[k].r[3] * pr[3]) < 0.0f ? -1.0f : 1.0f;
    float br[4], bd[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        br[c] = ((w[0] * (sg[0] * j[0].r[c]) + w[1] * (sg[1] * j[1].r[c])) + w[2] * (sg[2] * j[2].r[c])) + w[3] * (sg[3] * j[3].r[c]);
        bd[c] = ((w[0] * (sg[0] * j[0].d[c]) + w[1] * (sg[1] * j[1].d[c])) + w[2] * (sg[2] * j[2].d[c])) + w[3] * (sg[3] * j[3].d[c]);
    }
    const float sb = ((w[0] * j[0].s + w[1] * j[1].s) + w[2] * j[2].s) + w[3] * j[3].s;
    const float inv = rsqrt_exact(((br[0] * br[0] + br[1] * br[1]) + br[2] * br[2]) + br[3] * br[3]);
    const f3 u = mk3(br[0] * inv, br[1] * inv, br[2] * inv), d = mk3(bd[0] * inv, bd[1] * inv, bd[2] * inv);
    const float rw = br[3] * inv, dw = bd[3] * inv;
    const f3 v = mk3(sb * p[0], sb * p[1], sb * p[2]);
    const f3 rot = v + 2.0f * cross(u, cross(u, v) + rw * v);
    const f3 tr = 2.0f * ((rw * d - dw * u) + cross(u, d));
    out[0] = rot.x + tr.x; out[1] = rot.y + tr.y; out[2] = rot.z + tr.z;
    out[3] = p[3];
}

// The device pass is pose_batch_skin_dq_kernel (frt_pose_batch.hip): the loads and the store of pose_batch_skin_kernel; each of the vertex's four joints
// is converted in the lane as its columns arrive (skin_dq_of_joint), so one matrix is live at a time, and skinned_position_dq blends the four.

} // namespace frt
