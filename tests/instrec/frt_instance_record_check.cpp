// Host instantiation of csrc/frt_instance_record.hpp (the arithmetic the device-input set_instance_transforms kernels run) for
// tests/test_instance_transform_device.py, which compiles this file on its own with the library's contract flags and compares the results, bit for bit,
// with what the library's host functions (frt_scene.cpp) leave in a scene. Test infrastructure only.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_instance_record.hpp"
#include <string.h>

extern "C" {

// For each of the n column-major 4x4 in `mats`: ok[k] (0: non-finite or singular, nothing else written for k), w2o[9k..], flip[k], and the quad and
// sphere light records (16 words each) under the emissions em_quad / em_sphere.
void irc_batch(uint32_t n, const float* mats, const float* em_quad, const float* em_sphere, uint8_t* ok, float* w2o, uint32_t* flip, uint32_t* quad, uint32_t* sphere) {
    for (uint32_t k = 0; k < n; ++k) {
        const float* m = mats + 16 * (size_t)k;
        ok[k] = frt::record_instance_inverse(m, w2o + 9 * (size_t)k, flip[k]) ? 1 : 0;
        if (!ok[k]) continue;
        const frt::LightRecord q = frt::record_quad_light(m, em_quad), s = frt::record_sphere_light(m, em_sphere);
        memcpy(quad + 16 * (size_t)k, &q, 64);
        memcpy(sphere + 16 * (size_t)k, &s, 64);
    }
}

} // extern "C"
