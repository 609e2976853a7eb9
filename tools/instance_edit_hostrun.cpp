// instance_edit_hostrun.cpp — the host form of adding and removing instances (frt_scene_add_instances / _remove_instances) in a loop, as a
// stand-alone program to run under a sanitiser: it links the host scene sources only (no device code, nothing loaded into an interpreter).
//   hipcc --cuda-host-only -x hip -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Iinclude \
//       tools/instance_edit_hostrun.cpp fast-raytracing-wgpu_amd/csrc/frt_scene.cpp fast-raytracing-wgpu_amd/csrc/frt_bvh.cpp \
//       -fsanitize=address,undefined -o instance_edit_hostrun && ./instance_edit_hostrun
// (host only: frt_math.hpp wants the HIP headers, hence hipcc.) Exit status 0 and "ok" when every step behaved. Run it on a CPU machine.
#include "../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace frt;

static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what); exit(1); }
}
static bool same(const SceneBuilder& a, const SceneBuilder& b) {
    auto eq = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0); };
    return eq(a.tris, b.tris) && eq(a.tri_instance, b.tri_instance) && eq(a.bvh2, b.bvh2) && eq(a.bvh2_tri_index, b.bvh2_tri_index) && eq(a.quad_nodes, b.quad_nodes) &&
           eq(a.pair_nodes, b.pair_nodes) && eq(a.tri_slots, b.tri_slots) && eq(a.tri_slot_of, b.tri_slot_of) && eq(a.shade_tris, b.shade_tris) &&
           eq(a.instances_dev, b.instances_dev) && eq(a.lights, b.lights) && eq(a.materials, b.materials);
}

int main() {
    SceneBuilder s;
    scenes::create_cornell_box(s);
    expect(s.built, "the Cornell Box builds");
    SceneBuilder ref;
    scenes::create_cornell_box(ref);
    const size_t n0 = s.instances.size(), t0 = s.tris.size();
    uint32_t seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 24; ++round) {
        // add one to three instances of random meshes ...
        const uint32_t n = 1u + rnd() % 3u;
        uint32_t mesh[3], mat[3]; float m[48];
        for (uint32_t k = 0; k < n; ++k) {
            mesh[k] = rnd() % (uint32_t)s.mesh_infos.size(); mat[k] = rnd() % (uint32_t)s.materials.size();
            const Mat4 t = mat4_mul(mat4_mul(mat4_translation((float)(rnd() % 100) * 0.01f - 0.5f, (float)(rnd() % 100) * 0.01f - 0.5f, (float)(rnd() % 100) * 0.01f - 0.5f),
                                             mat4_rotation_y((float)(rnd() % 628) * 0.01f)), mat4_scale(0.2f, 0.3f, 0.25f));
            memcpy(m + 16 * k, t.m, 64);
        }
        const int first = s.add_instances(n, mesh, mat, m);
        expect(first == (int)s.instances.size() - (int)n && s.built, "add_instances returns the first new id");
        s.ensure_wide8();
        // ... refusals in between (out of range, singular, a registered light, everything) ...
        const uint32_t bad_mesh = (uint32_t)s.mesh_infos.size(), zero = 0u;
        float flat[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        expect(s.add_instances(1, &bad_mesh, &zero, m) == FRT_ERR_INVALID_ARG, "mesh id out of range");
        expect(s.add_instances(1, &zero, &zero, flat) == FRT_ERR_INVALID_ARG, "singular matrix");
        expect(s.add_instances(1, nullptr, &zero, m) == FRT_ERR_INVALID_ARG, "null pointer");
        const uint32_t light = 5u, beyond = (uint32_t)s.instances.size();
        expect(s.remove_instances(1, &light) == FRT_ERR_INVALID_ARG, "a registered-light instance");
        expect(s.remove_instances(1, &beyond) == FRT_ERR_INVALID_ARG, "instance id out of range");
        // ... and remove what was added, in reverse order with a duplicate, plus (every third round) an original one that is put back
        uint32_t ids[4]; uint32_t k = 0;
        for (uint32_t j = n; j-- > 0;) ids[k++] = (uint32_t)first + j;
        ids[k++] = (uint32_t)first;
        expect(s.remove_instances(k, ids) == FRT_OK, "remove_instances");
        expect(s.instances.size() == n0 && s.tris.size() == t0, "the counts are back");
        if (round % 3 == 0) {
            const uint32_t last = (uint32_t)n0 - 1u;
            const InstanceRec was = s.instances[last];
            expect(s.remove_instances(1, &last) == FRT_OK, "remove the last original instance");
            expect(s.add_instances(1, &was.mesh_id, &was.mat_id, was.m) == (int)last, "put it back");
        }
        expect(same(s, ref), "the scene equals the one built from scratch");
    }
    SceneBuilder unbuilt;
    const uint32_t z = 0u;
    expect(unbuilt.add_instances(0, nullptr, nullptr, nullptr) == FRT_ERR_STATE && unbuilt.remove_instances(1, &z) == FRT_ERR_STATE, "not built");
    puts("ok");
    return 0;
}
