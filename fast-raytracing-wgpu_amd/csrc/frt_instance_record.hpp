// frt_instance_record.hpp — what a new instance matrix makes of an instance's records ("Transforms from device memory"): world_to_object
// and flip by cofactors in double, and the light record of an instance that register_quad_light / register_sphere_light created. A restatement of
// cofactor_inverse, instance_inverse, quad_light_record and sphere_light_record (frt_scene.cpp), which stay the specification and are what the tests
// compare these against, bit for bit: the same operations in the same order, no contraction, no hand-written fma, IEEE division and square root.
// __host__ __device__, and free of every other header of the library, so that a stand-alone host program can compile it with a plain C++ compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRT_REC_HD __host__ __device__ inline
#else
#define FRT_REC_HD inline
#endif

namespace frt {

struct LightRecord { float position[3]; uint32_t type_; float u[3]; float area; float v[3]; uint32_t pad; float emission[4]; };   // = frt_light, LightView (64 B)
static_assert(sizeof(LightRecord) == 64, "LightRecord layout");

FRT_REC_HD bool record_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

// cofactor_inverse: the inverse of the 3x3 of the column-major `m` (m[4c + r]) in double, rounded once to f32 (w2o[3c + r]); returns the determinant.
FRT_REC_HD double record_cofactor_inverse(const float m[16], float w2o[9], uint32_t& flip) {
    double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    double k00 = e * i - f * h, k01 = f * g - d * i, k02 = d * h - e * g;
    double det = a * k00 + b * k01 + c * k02;
    double inv[3][3] = {{k00 / det, (c * h - b * i) / det, (b * f - c * e) / det},
                        {k01 / det, (a * i - c * g) / det, (c * d - a * f) / det},
                        {k02 / det, (b * g - a * h) / det, (a * e - b * d) / det}};
    for (int col = 0; col < 3; ++col) for (int row = 0; row < 3; ++row) w2o[3 * col + row] = (float)inv[row][col];
    flip = det < 0.0 ? 1u : 0u;
    return det;
}
// instance_inverse: false (outputs untouched) when the matrix has a non-finite entry or a singular 3x3.
FRT_REC_HD bool record_instance_inverse(const float m[16], float w2o[9], uint32_t& flip) {
    for (int k = 0; k < 16; ++k) if (!record_finite(m[k])) return false;
    float w[9]; uint32_t fl;
    if (!(record_cofactor_inverse(m, w, fl) != 0.0)) return false;
    for (int k = 0; k < 9; ++k) w2o[k] = w[k];
    flip = fl;
    return true;
}

// xform_vec3 (glam transform_vector3): the 3x3 of `m` times (x, y, z).
FRT_REC_HD void record_xform_vec3(const float m[16], float x, float y, float z, float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = (m[i] * x + m[4 + i] * y) + m[8 + i] * z;
}
// quad_light_record: the plane mesh spans (+-1, 0, +-1); u and v are its half edges, area = |(2u) x (2v)|.
FRT_REC_HD LightRecord record_quad_light(const float m[16], const float emission[4]) {
    float u[3], v[3];
    record_xform_vec3(m, 1, 0, 0, u); record_xform_vec3(m, 0, 0, -1, v);
    for (int i = 0; i < 3; ++i) { u[i] *= 0.5f; v[i] *= 0.5f; }
    float cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    LightRecord l = {};
    for (int i = 0; i < 3; ++i) { l.position[i] = m[12 + i]; l.u[i] = u[i]; l.v[i] = v[i]; }
    for (int i = 0; i < 4; ++i) l.emission[i] = emission[i];
    l.type_ = 0;
    l.area = __builtin_sqrtf(cx * cx + cy * cy + cz * cz) * 4.0f;
    return l;
}
// sphere_light_record: radius = half the length of the transformed x axis (v[0]), area = 4 pi r^2.
FRT_REC_HD LightRecord record_sphere_light(const float m[16], const float emission[4]) {
    float x[3];
    record_xform_vec3(m, 1, 0, 0, x);
    float scale = __builtin_sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    float radius = scale * 0.5f;
    LightRecord l = {};
    for (int i = 0; i < 3; ++i) l.position[i] = m[12 + i];
    for (int i = 0; i < 4; ++i) l.emission[i] = emission[i];
    l.type_ = 1;
    l.area = 4.0f * 3.14159265358979323846f * radius * radius;
    l.v[0] = radius;
    return l;
}

} // namespace frt
