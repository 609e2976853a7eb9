// morph_hostrun.cpp — the host half of the morph targets ("Morph targets") as a stand-alone program to run under a sanitiser: the argument
// checks of frt_scene.cpp (check_mesh_morph_targets, check_mesh_morph_weights), frt_morph.hpp's morphed_position compiled for the host, and the scene
// forms set_mesh_morph_targets / set_mesh_morph_weights / set_mesh_pose_ex against scenes given the same positions through set_mesh_vertices. It links the
// host scene sources only (no device code, nothing loaded into an interpreter).
//   hipcc --cuda-host-only -x hip -std=c++17 -g -O1 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/morph_hostrun.cpp fast-raytracing-wgpu_amd/csrc/frt_scene.cpp fast-raytracing-wgpu_amd/csrc/frt_bvh.cpp \
//       -fsanitize=address,undefined -o morph_hostrun && ./morph_hostrun
// Exit status 0 and "ok" when every step behaved. Run it on a CPU machine.
#include "../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include "../fast-raytracing-wgpu_amd/csrc/frt_morph.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace frt;

static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what); exit(1); }
}
template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static void expect_same(const SceneBuilder& a, const SceneBuilder& b, const char* what) {
    expect(a.built && b.built, what);
    expect(a.mesh_positions == b.mesh_positions && same(a.attributes, b.attributes) && same(a.tris, b.tris) && same(a.tri_slots, b.tri_slots) &&
           same(a.shade_tris, b.shade_tris) && same(a.quad_nodes, b.quad_nodes), what);
}

// A floor, an unused crystal (mesh 1) and a cube (mesh 2).
static void make(SceneBuilder& b) {
    const uint32_t plane = b.add_mesh(geometry::create_plane());
    b.add_mesh(geometry::create_crystal());
    const uint32_t cube = b.add_mesh(geometry::create_cube());
    const uint32_t grey = b.add_material(MaterialBuilder(0.7f, 0.7f, 0.7f, 1.0f));
    const float white[3] = {1.0f, 1.0f, 1.0f};
    b.register_quad_light(plane, mat4_mul(mat4_translation(0.0f, 1.0f, 0.0f), mat4_rotation_x(3.14159265f)), white, 5.0f);
    b.add_instance(plane, grey, mat4_scale(3.0f, 3.0f, 3.0f));
    b.add_instance(cube, grey, mat4_mul(mat4_translation(-0.4f, 0.3f, 0.1f), mat4_scale(0.5f, 0.5f, 0.5f)));
    b.build();
}
static std::vector<float> deltas_for(uint32_t nverts, uint32_t ntargets) {
    std::vector<float> d((size_t)ntargets * nverts * 3);
    for (size_t k = 0; k < d.size(); ++k) d[k] = 0.01f * (float)((int)(k * 7919u % 13u) - 6);
    return d;
}
// The contract, written out again: a loop over the targets in order.
static std::vector<float> model(const std::vector<float>& base, const std::vector<float>& d, const std::vector<float>& w) {
    const size_t n = base.size() / 4;
    std::vector<float> out = base;
    for (size_t t = 0; t < w.size(); ++t)
        for (size_t v = 0; v < n; ++v)
            for (int r = 0; r < 3; ++r) { const float term = w[t] * d[(t * n + v) * 3 + r]; out[4 * v + r] = out[4 * v + r] + term; }
    return out;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the checks
    {
        std::vector<float> d = deltas_for(5, 3), w = {0.0f, -0.5f, 1.5f};
        expect(check_mesh_morph_targets(d.data(), 5, 3, 5).empty(), "good targets");
        expect(!check_mesh_morph_targets(nullptr, 5, 3, 5).empty() && !check_mesh_morph_targets(d.data(), 4, 3, 5).empty(), "null deltas, a wrong vertex count");
        expect(!check_mesh_morph_targets(d.data(), 5, 0, 5).empty() && !check_mesh_morph_targets(d.data(), 5, FRT_MAX_MORPH_TARGETS + 1u, 5).empty(), "no targets, too many (no delta is read)");
        d.back() = inf;
        expect(!check_mesh_morph_targets(d.data(), 5, 3, 5).empty(), "the last delta is infinite");
        d.back() = 0.0f; d[0] = nan;
        expect(!check_mesh_morph_targets(d.data(), 5, 3, 5).empty(), "the first delta is a NaN");
        expect(check_mesh_morph_weights(w.data(), 3, 3).empty(), "good weights");
        expect(!check_mesh_morph_weights(w.data(), 3, 0).empty() && !check_mesh_morph_weights(w.data(), 2, 3).empty() && !check_mesh_morph_weights(nullptr, 3, 3).empty(), "no targets, a wrong count, null");
        w[2] = -inf;
        expect(!check_mesh_morph_weights(w.data(), 3, 3).empty() && check_mesh_morph_weights(w.data(), 3, 3, false).empty(), "a non-finite weight; device memory is not read");
    }
    // the arithmetic: target counts around the unroll of four
    for (uint32_t T : {1u, 3u, 4u, 5u, 70u}) {
        SceneBuilder s, ref;
        make(s); make(ref);
        const std::vector<float> base = s.mesh_positions[2];
        const uint32_t n = (uint32_t)(base.size() / 4);
        const std::vector<float> d = deltas_for(n, T);
        std::vector<float> w(T);
        for (uint32_t t = 0; t < T; ++t) w[t] = t == 0 ? 0.0f : (t % 2 ? -0.375f : 1.25f) + 0.01f * (float)t;
        if (T == 1) w[0] = 1.25f;
        expect(s.set_mesh_morph_weights(2, w.data(), T, 0) == FRT_ERR_INVALID_ARG, "no targets yet");
        expect(s.set_mesh_morph_targets(2, d.data(), n, T) == FRT_OK, "bind");
        expect_same(s, ref, "binding changes nothing");
        expect(s.set_mesh_morph_weights(2, w.data(), T, FRT_DEFORM_RECOMPUTE_NORMALS) == FRT_OK, "morph");
        const std::vector<float> m = model(base, d, w);
        expect(ref.set_mesh_vertices(2, m.data(), nullptr, n, FRT_DEFORM_RECOMPUTE_NORMALS) == FRT_OK, "reference");
        expect_same(s, ref, "a morph equals set_mesh_vertices with the model's positions");
        expect(s.set_mesh_morph_weights(2, w.data(), T, 0) == FRT_OK && s.mesh_positions[2] == m, "a second morph starts from the base");
        // refusals
        expect(s.set_mesh_morph_weights(2, w.data(), T + 1, 0) == FRT_ERR_INVALID_ARG && s.set_mesh_morph_weights(9, w.data(), T, 0) == FRT_ERR_INVALID_ARG, "a wrong count, a wrong mesh");
        expect(s.set_mesh_morph_weights(2, w.data(), T, 4u) == FRT_ERR_INVALID_ARG && s.set_mesh_morph_weights(2, w.data(), T, FRT_DEFORM_DEVICE) == FRT_ERR_INVALID_ARG, "flags");
        std::vector<float> bad = w; bad[T - 1] = nan;
        expect(s.set_mesh_morph_weights(2, bad.data(), T, 0) == FRT_ERR_INVALID_ARG, "a NaN weight");
        std::vector<float> big(d.size(), 1.0e36f), huge(T, 1.0e3f);
        expect(s.set_mesh_morph_targets(2, big.data(), n, T) == FRT_OK && s.set_mesh_morph_weights(2, huge.data(), T, 0) == FRT_ERR_INVALID_ARG, "finite inputs that overflow");
        expect(s.mesh_positions[2] == m, "refusals change nothing");
        // morph, then skin: two joints, joint 1 lifts by one half
        expect(s.set_mesh_morph_targets(2, nullptr, 0, 0) == FRT_OK && s.set_mesh_vertices(2, base.data(), nullptr, n, 0) == FRT_OK && s.set_mesh_morph_targets(2, d.data(), n, T) == FRT_OK, "bound again at rest");
        std::vector<uint16_t> joints((size_t)n * 4, 0);
        std::vector<float> sw((size_t)n * 4, 0.0f), mats(32, 0.0f);
        for (uint32_t v = 0; v < n; ++v) { joints[4 * v + 1] = 1; sw[4 * v] = 0.25f * (float)(v % 5); sw[4 * v + 1] = 1.0f - sw[4 * v]; }
        for (int j = 0; j < 2; ++j) for (int c = 0; c < 4; ++c) mats[16 * j + 5 * c] = 1.0f;
        mats[16 + 13] = 0.5f;
        expect(s.set_mesh_pose_ex(2, mats.data(), 2, w.data(), T, 0) == FRT_ERR_INVALID_ARG, "no skin yet");
        expect(s.set_mesh_skin(2, joints.data(), sw.data(), n, 2) == FRT_OK, "skin");
        expect(s.set_mesh_pose_ex(2, mats.data(), 2, w.data(), T, 0) == FRT_OK, "morph and skin");
        SceneBuilder two;
        make(two);
        expect(two.set_mesh_vertices(2, m.data(), nullptr, n, 0) == FRT_OK && two.set_mesh_skin(2, joints.data(), sw.data(), n, 2) == FRT_OK && two.set_mesh_pose(2, mats.data(), 2, 0) == FRT_OK, "skin over the morphed mesh");
        expect(s.mesh_positions[2] == two.mesh_positions[2] && same(s.tri_slots, two.tri_slots), "the combined call skins the morphed positions");
        expect(s.set_mesh_pose_ex(2, mats.data(), 2, nullptr, T, 0) == FRT_ERR_INVALID_ARG && s.set_mesh_pose_ex(2, mats.data(), 2, w.data(), 0, 0) == FRT_ERR_INVALID_ARG, "half a morph input");
        expect(s.set_mesh_pose_ex(2, mats.data(), 2, nullptr, 0, 0) == FRT_OK, "without weights: set_mesh_pose");
        // the targets follow remove_meshes
        const uint32_t one = 1;
        expect(s.remove_meshes(1, &one) == FRT_OK && s.mesh_morphs.size() == 2 && s.mesh_morphs[1].ntargets == T, "the cube's targets follow it to id 1");
        expect(s.set_mesh_morph_weights(1, w.data(), T, 0) == FRT_OK && s.mesh_positions[1] == m, "and morph it there");
        expect(s.set_mesh_morph_weights(0, w.data(), T, 0) == FRT_ERR_INVALID_ARG, "the plane has none");
    }
    SceneBuilder unbuilt;
    const float z[3] = {0.0f, 0.0f, 0.0f};
    expect(unbuilt.set_mesh_morph_targets(0, z, 1, 1) == FRT_ERR_STATE && unbuilt.set_mesh_morph_weights(0, z, 1, 0) == FRT_ERR_STATE && unbuilt.set_mesh_pose_ex(0, z, 1, z, 1, 0) == FRT_ERR_STATE, "not built");
    printf("ok\n");
    return 0;
}
