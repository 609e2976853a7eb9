// ik_sanitize.cpp — the host form of inverse kinematics on a rig (csrc/frt_animation.cpp: frt_rig_evaluate_layers_ik, frt_rig_evaluate_nodes_layers_ik)
// stand-alone, for a build with -fsanitize=address,undefined (tests/test_animation_ik.py builds it with the command line of layers_sanitize.cpp).
// Every array is a heap block of exactly the size the call may touch, so a read or a write past it is seen; every refusal is made with the outputs
// filled with a sentinel, which must still be there afterwards. Prints "ok: ..." and returns 0, or says what went wrong.
#include "../include/frt.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace frt { int set_error(int code, const std::string& msg) { (void)msg; return code; } }

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) { std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]); if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T)); return p; }

int main() {
    // a chain of five nodes, unit bones along y, two clips (one turns node 1), every node a joint
    const uint32_t N = 5;
    std::vector<int32_t> parents = {-1, 0, 1, 2, 3};
    std::vector<float> trs(10 * N, 0.0f);
    for (uint32_t n = 0; n < N; ++n) { trs[10 * n + 1] = n ? 1.0f : 0.0f; trs[10 * n + 6] = 1.0f; trs[10 * n + 7] = trs[10 * n + 8] = trs[10 * n + 9] = 1.0f; }
    std::vector<uint32_t> joints = {0, 1, 2, 3, 4};
    const float times[2] = {0.0f, 1.0f};
    const float rot[8] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.38268343f, 0.92387953f};
    frt_rig_channel ch{1u, 1u, 1u, 2u, times, rot};
    frt_rig_clip clips[2] = {{"rest", 0u, nullptr}, {"turn", 1u, &ch}};
    frt_rig_desc d;
    memset(&d, 0, sizeof(d));
    d.nnodes = N; d.parents = parents.data(); d.rest_trs = trs.data(); d.njoints = N; d.joint_nodes = joints.data(); d.nclips = 2; d.clips = clips;
    frt_rig* rig = frt_rig_create(&d);
    if (!rig) { printf("rig_create failed\n"); return 1; }
    std::vector<frt_clip_layer> layers = {{0u, 0.0f, 1.0f, FRT_LAYER_NO_MASK, FRT_LAYER_BLEND, 0u, 0.0f, 0u}, {1u, 0.5f, 0.5f, FRT_LAYER_NO_MASK, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u}};
    std::vector<frt_rig_goal> goals = {{FRT_GOAL_TWO_BONE, 0u, 2u, 4u, {0.0f, 0.0f, 0.0f}, 0u}, {FRT_GOAL_AIM, 4u, 0u, 0u, {0.0f, 1.0f, 0.0f}, 0u}, {FRT_GOAL_TWO_BONE, 1u, 2u, 3u, {0.0f, 0.0f, 0.0f}, 0u}};
    std::vector<frt_rig_goal_target> targets = {{{1.5f, 1.0f, 0.5f}, 1.0f, {0.0f, 0.0f, 2.0f}, 1.0f}, {{3.0f, 3.0f, 0.0f}, 0.5f, {0.0f, 0.0f, 0.0f}, 0.0f}, {{0.5f, 1.5f, 0.2f}, 0.75f, {0.0f, 0.0f, 0.0f}, 0.0f}};
    std::vector<uint32_t> nodes = {4u, 0u, 2u};
    const float kSentinel = 7.0f;
    std::vector<float> pal(16 * N, kSentinel), mats(16 * nodes.size(), kSentinel);
    auto L = exact(layers); auto G = exact(goals); auto T = exact(targets); auto Q = exact(nodes); auto P = exact(pal); auto M = exact(mats);
    auto untouched = [&]() { for (size_t i = 0; i < pal.size(); ++i) if (P[i] != kSentinel) return false; for (size_t i = 0; i < mats.size(); ++i) if (M[i] != kSentinel) return false; return true; };
    int refusals = 0;
    auto refuse = [&](const char* what, uint32_t ng, const frt_rig_goal* g, const frt_rig_goal_target* t) {
        const int a = frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, ng, g, t, P.get(), nullptr);
        const int b = frt_rig_evaluate_nodes_layers_ik(rig, 2u, L.get(), 0u, nullptr, ng, g, t, 3u, Q.get(), nullptr, nullptr, M.get());
        if (a != FRT_ERR_INVALID_ARG || b != FRT_ERR_INVALID_ARG || !untouched()) { printf("not refused, or an output written: %s\n", what); return false; }
        ++refusals;
        return true;
    };
    auto with_goal = [&](const char* what, size_t i, frt_rig_goal g) { std::vector<frt_rig_goal> v = goals; v[i] = g; auto p = exact(v); return refuse(what, 3u, p.get(), T.get()); };
    auto with_target = [&](const char* what, size_t i, frt_rig_goal_target t) { std::vector<frt_rig_goal_target> v = targets; v[i] = t; auto p = exact(v); return refuse(what, 3u, G.get(), p.get()); };
    const float nan = std::nanf(""), inf = INFINITY;
    bool ok = refuse("more than FRT_MAX_RIG_GOALS", 17u, G.get(), T.get()) && refuse("a huge count", 0xFFFFFFFFu, G.get(), T.get()) && refuse("null goals", 3u, nullptr, T.get()) &&
              refuse("null targets", 3u, G.get(), nullptr) &&
              with_goal("an unknown kind", 0, {3u, 0u, 2u, 4u, {0, 0, 0}, 0u}) && with_goal("reserved", 1, {FRT_GOAL_AIM, 4u, 0u, 0u, {0, 1, 0}, 1u}) &&
              with_goal("a node out of range", 0, {FRT_GOAL_TWO_BONE, 0u, 2u, 5u, {0, 0, 0}, 0u}) && with_goal("mid is root", 0, {FRT_GOAL_TWO_BONE, 2u, 2u, 4u, {0, 0, 0}, 0u}) &&
              with_goal("mid above root", 0, {FRT_GOAL_TWO_BONE, 2u, 1u, 4u, {0, 0, 0}, 0u}) && with_goal("tip is mid", 2, {FRT_GOAL_TWO_BONE, 1u, 3u, 3u, {0, 0, 0}, 0u}) &&
              with_goal("tip above mid", 2, {FRT_GOAL_TWO_BONE, 1u, 3u, 2u, {0, 0, 0}, 0u}) && with_goal("a zero axis", 1, {FRT_GOAL_AIM, 4u, 0u, 0u, {0, 0, 0}, 0u}) &&
              with_goal("a NaN axis", 1, {FRT_GOAL_AIM, 4u, 0u, 0u, {0, nan, 0}, 0u}) && with_goal("an aim with a mid", 1, {FRT_GOAL_AIM, 4u, 1u, 0u, {0, 1, 0}, 0u}) &&
              with_goal("an aim with a tip", 1, {FRT_GOAL_AIM, 4u, 0u, 1u, {0, 1, 0}, 0u}) && with_goal("an aim node out of range", 1, {FRT_GOAL_AIM, 5u, 0u, 0u, {0, 1, 0}, 0u}) &&
              with_target("a NaN target", 0, {{nan, 1.0f, 0.5f}, 1.0f, {0, 0, 2.0f}, 1.0f}) && with_target("an infinite pole", 0, {{1.5f, 1.0f, 0.5f}, 1.0f, {0, inf, 2.0f}, 1.0f}) &&
              with_target("a weight above 1", 2, {{0.5f, 1.5f, 0.2f}, 1.5f, {0, 0, 0}, 0.0f}) && with_target("a negative weight", 2, {{0.5f, 1.5f, 0.2f}, -0.5f, {0, 0, 0}, 0.0f}) &&
              with_target("a NaN weight", 2, {{0.5f, 1.5f, 0.2f}, nan, {0, 0, 0}, 0.0f}) && with_target("a pole flag of 2", 0, {{1.5f, 1.0f, 0.5f}, 1.0f, {0, 0, 2.0f}, 2.0f}) &&
              with_target("a pole on an aim", 1, {{3.0f, 3.0f, 0.0f}, 0.5f, {0, 0, 0}, 1.0f}) && with_target("a pole word on an aim", 1, {{3.0f, 3.0f, 0.0f}, 0.5f, {0, 0.5f, 0}, 0.0f});
    if (!ok) return 1;
    // the good calls write every output, finite; no goals is the layered call bit for bit; weights of zero are no goals
    if (frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, 3u, G.get(), T.get(), P.get(), nullptr) != FRT_OK) { printf("evaluate_layers_ik failed\n"); return 1; }
    if (frt_rig_evaluate_nodes_layers_ik(rig, 2u, L.get(), 0u, nullptr, 3u, G.get(), T.get(), 3u, Q.get(), nullptr, nullptr, M.get()) != FRT_OK) { printf("evaluate_nodes_layers_ik failed\n"); return 1; }
    for (size_t i = 0; i < pal.size(); ++i) if (P[i] == kSentinel || !std::isfinite(P[i])) { printf("palette entry %zu not written or not finite\n", i); return 1; }
    for (size_t i = 0; i < mats.size(); ++i) if (M[i] == kSentinel || !std::isfinite(M[i])) { printf("matrix entry %zu not written or not finite\n", i); return 1; }
    if (memcmp(M.get(), P.get() + 16 * 4, 64) != 0) { printf("the node form and the palette disagree on node 4\n"); return 1; }
    std::vector<float> plain(16 * N), none(16 * N), zero(16 * N);
    std::vector<frt_rig_goal_target> z = targets;
    for (frt_rig_goal_target& t : z) t.weight = 0.0f;
    auto Z = exact(z);
    if (frt_rig_evaluate_layers(rig, 2u, L.get(), 0u, nullptr, plain.data(), nullptr) != FRT_OK || frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, 0u, nullptr, nullptr, none.data(), nullptr) != FRT_OK ||
        frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, 3u, G.get(), Z.get(), zero.data(), nullptr) != FRT_OK) { printf("a plain call failed\n"); return 1; }
    if (memcmp(plain.data(), none.data(), plain.size() * 4) != 0 || memcmp(plain.data(), zero.data(), plain.size() * 4) != 0) { printf("no goals or zero weights differ from the layered call\n"); return 1; }
    if (memcmp(plain.data(), P.get(), plain.size() * 4) == 0) { printf("the goals changed nothing\n"); return 1; }
    // sixteen goals, the most a call takes
    std::vector<frt_rig_goal> many; std::vector<frt_rig_goal_target> many_t;
    for (uint32_t i = 0; i < FRT_MAX_RIG_GOALS; ++i) { many.push_back(goals[i % 3]); many_t.push_back(targets[i % 3]); }
    auto MG = exact(many); auto MT = exact(many_t);
    if (frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, FRT_MAX_RIG_GOALS, MG.get(), MT.get(), P.get(), nullptr) != FRT_OK) { printf("sixteen goals failed\n"); return 1; }
    frt_rig_destroy(rig);
    printf("ok: %d refusals with the outputs untouched, both evaluations with exactly sized arrays\n", refusals);
    return 0;
}
