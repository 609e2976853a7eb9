// skin_dq_sanitize.cpp — the host form of dual-quaternion skinning (csrc/frt_skin.hpp: skin_dq_of_joint, skinned_position_dq; csrc/frt_scene.cpp:
// set_mesh_skin with FRT_SKIN_DUAL_QUATERNION, set_mesh_pose, set_mesh_poses) stand-alone, for a build with -fsanitize=address,undefined
// (tests/test_mesh_skin_dq.py builds it with the command line of ik_sanitize.cpp, against frt_scene.cpp and frt_bvh.cpp). Every array handed to a
// call is a heap block of exactly the size the call may touch, so a read past it is seen; every refusal must leave the scene as it was. Prints
// "ok: ..." and returns 0, or says what went wrong.
#include "../fast-raytracing-wgpu_amd/csrc/frt_scene.hpp"
#include "../fast-raytracing-wgpu_amd/csrc/frt_skin.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace frt;

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) { std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]); if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T)); return p; }
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

// A floor and a cube (mesh 1, 24 vertices), as tools/morph_hostrun.cpp builds them.
static void make(SceneBuilder& b) {
    const uint32_t plane = b.add_mesh(geometry::create_plane());
    const uint32_t cube = b.add_mesh(geometry::create_cube());
    const uint32_t grey = b.add_material(MaterialBuilder(0.7f, 0.7f, 0.7f, 1.0f));
    const float white[3] = {1.0f, 1.0f, 1.0f};
    b.register_quad_light(plane, mat4_mul(mat4_translation(0.0f, 1.0f, 0.0f), mat4_rotation_x(3.14159265f)), white, 5.0f);
    b.add_instance(plane, grey, mat4_scale(3.0f, 3.0f, 3.0f));
    b.add_instance(cube, grey, mat4_mul(mat4_translation(-0.4f, 0.3f, 0.1f), mat4_scale(0.5f, 0.5f, 0.5f)));
    b.build();
}
static std::vector<float> turn_y(float angle, float tx, float s) {      // column-major T(tx, 0, 0) R_y(angle) S(s)
    const float c = cosf(angle), n = sinf(angle);
    return {s * c, 0.0f, -s * n, 0.0f, 0.0f, s, 0.0f, 0.0f, s * n, 0.0f, s * c, 0.0f, tx, 0.0f, 0.0f, 1.0f};
}

int main() {
    SceneBuilder s;
    make(s);
    const uint32_t cube = 1, n = (uint32_t)(s.mesh_positions[cube].size() / 4), J = 3;
    std::vector<uint16_t> joints((size_t)n * 4);
    std::vector<float> weights((size_t)n * 4);
    for (uint32_t v = 0; v < n; ++v) {
        for (int k = 0; k < 4; ++k) joints[4 * v + k] = (uint16_t)((v + (uint32_t)k) % 2u);      // joints 0 and 1 are named, joint 2 by no vertex
        const float a = 0.125f * (float)(v % 8u);
        weights[4 * v] = a; weights[4 * v + 1] = 1.0f - a; weights[4 * v + 2] = v % 3u ? 0.0f : 0.25f; weights[4 * v + 3] = 0.0f;
    }
    std::vector<float> pal;
    for (const std::vector<float>& m : {turn_y(0.4f, 0.1f, 1.0f), turn_y(2.9f, -0.2f, 1.5f), turn_y(-1.0f, 0.0f, 0.5f)}) pal.insert(pal.end(), m.begin(), m.end());
    auto Jp = exact(joints); auto Wp = exact(weights); auto Pp = exact(pal);
    int refusals = 0;
    // the bind call: an unknown flag bit changes nothing, in front of and behind a good bind
    if (s.set_mesh_skin(cube, Jp.get(), Wp.get(), n, J, 2u) != FRT_ERR_INVALID_ARG || s.set_mesh_skin(cube, Jp.get(), Wp.get(), n, J, 3u) != FRT_ERR_INVALID_ARG) return fail("an unknown flag bit");
    refusals += 2;
    if (!s.mesh_skins.empty() && s.mesh_skins.size() > cube && s.mesh_skins[cube].njoints) return fail("a refused bind left a skin");
    if (s.set_mesh_skin(cube, Jp.get(), Wp.get(), n, J, FRT_SKIN_DUAL_QUATERNION) != FRT_OK || s.mesh_skins[cube].mode != FRT_SKIN_DUAL_QUATERNION) return fail("bind");
    if (s.set_mesh_skin(cube, Jp.get(), Wp.get(), n, J, 4u) != FRT_ERR_INVALID_ARG || s.mesh_skins[cube].mode != FRT_SKIN_DUAL_QUATERNION) return fail("an unknown bit over a bound skin");
    ++refusals;
    // a pose, against the header's functions called here vertex by vertex
    const std::vector<float> bind = s.mesh_positions[cube];
    if (s.set_mesh_pose(cube, Pp.get(), J, FRT_DEFORM_RECOMPUTE_NORMALS) != FRT_OK) return fail("pose");
    for (uint32_t v = 0; v < n; ++v) {
        SkinDualQuat dq[4];
        for (int k = 0; k < 4; ++k) dq[k] = skin_dq_of_joint(Pp.get() + 16 * (size_t)joints[4 * v + k]);
        float o[4];
        skinned_position_dq(&bind[4 * v], dq, &weights[4 * v], o);
        if (memcmp(o, &s.mesh_positions[cube][4 * v], 16) != 0) return fail("the scene's pose is not the header's");
    }
    const std::vector<float> posed = s.mesh_positions[cube];
    const std::vector<TriSlot> slots = s.tri_slots;
    auto untouched = [&]() { return s.mesh_positions[cube] == posed && s.tri_slots.size() == slots.size() && memcmp(s.tri_slots.data(), slots.data(), slots.size() * sizeof(TriSlot)) == 0; };
    auto refuse = [&](const char* what, const std::vector<float>& p, uint32_t nj, uint32_t flags) {
        auto q = exact(p);
        const uint32_t ids[1] = {cube};
        if (s.set_mesh_pose(cube, q.get(), nj, flags) != FRT_ERR_INVALID_ARG || s.set_mesh_poses(1, ids, q.get(), nj, nullptr, 0, flags) != FRT_ERR_INVALID_ARG || !untouched()) {
            printf("not refused, or the scene changed: %s\n", what);
            return false;
        }
        refusals += 2;
        return true;
    };
    std::vector<float> bad = pal;
    bad[4] = bad[5] = bad[6] = 0.0f;
    if (!refuse("a zero column in a named joint", bad, J, 0u)) return 1;
    bad = pal; bad[16 + 9] = NAN;
    if (!refuse("a NaN entry", bad, J, 0u)) return 1;
    bad = pal; bad[32 + 12] = INFINITY;
    if (!refuse("an infinite entry in a joint no vertex names", bad, J, 0u)) return 1;
    bad = pal; for (int c = 0; c < 3; ++c) bad[4 * c + c] = 3.0e38f;
    if (!refuse("a column whose squared length overflows", bad, J, 0u)) return 1;
    if (!refuse("a palette of another size", std::vector<float>(pal.begin(), pal.begin() + 32), 2u, 0u)) return 1;
    if (!refuse("an unknown flag bit", pal, J, 4u)) return 1;
    if (!refuse("the device flag", pal, J, FRT_DEFORM_DEVICE)) return 1;
    bad = pal; bad[32] = bad[33] = bad[34] = 0.0f;      // a zero column in the joint no vertex names: nothing reads it
    { auto q = exact(bad); if (s.set_mesh_pose(cube, q.get(), J, 0u) != FRT_OK || s.mesh_positions[cube] != posed) return fail("an unnamed joint's zero column must not matter"); }
    // weights that are all zero: the blend is exactly zero, refused
    std::vector<float> zero((size_t)n * 4, 0.0f);
    auto Zp = exact(zero);
    if (s.set_mesh_vertices(cube, bind.data(), nullptr, n, 0u) != FRT_OK || s.set_mesh_skin(cube, Jp.get(), Zp.get(), n, J, FRT_SKIN_DUAL_QUATERNION) != FRT_OK) return fail("bind with zero weights");
    if (s.set_mesh_pose(cube, Pp.get(), J, 0u) != FRT_ERR_INVALID_ARG || s.mesh_positions[cube] != bind) return fail("a blend that cancels");
    ++refusals;
    // binding again replaces the mode; removing the skin drops it
    if (s.set_mesh_skin(cube, Jp.get(), Wp.get(), n, J, 0u) != FRT_OK || s.mesh_skins[cube].mode != 0u) return fail("a linear bind over a dual-quaternion one");
    if (s.set_mesh_skin(cube, nullptr, nullptr, 0, 0, 0u) != FRT_OK || s.mesh_skins[cube].njoints != 0u || s.mesh_skins[cube].mode != 0u) return fail("removing the skin");
    printf("ok: %d refusals left the scene untouched, %u vertices posed\n", refusals, n);
    return 0;
}
