// ik_chain_sanitize.cpp — chain IK on the host (csrc/frt_animation.cpp: frt_rig_evaluate_layers_ik, frt_rig_evaluate_nodes_layers_ik under
// FRT_GOAL_CHAIN goals) stand-alone, for a build with -fsanitize=address,undefined (tests/test_animation_ik_chain.py builds it with the command
// line of ik_sanitize.cpp). Every array is a heap block of exactly the size the call may touch, so a read or a write past it is seen; chains of 2
// and of 32 nodes, the shortest and the longest; every refusal is made with the outputs filled with a sentinel, which must still be there
// afterwards. Prints "ok: ..." and returns 0, or says what went wrong.
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
    // a chain of 34 nodes, unit bones along y, node 34 hanging off node 10 sideways; two clips (one turns node 1); every node a joint
    const uint32_t N = 35;
    std::vector<int32_t> parents(N);
    for (uint32_t n = 0; n < N; ++n) parents[n] = (int32_t)n - 1;
    parents[34] = 10;
    std::vector<float> trs(10 * N, 0.0f);
    for (uint32_t n = 0; n < N; ++n) { trs[10 * n + 1] = n ? 1.0f : 0.0f; trs[10 * n + 6] = 1.0f; trs[10 * n + 7] = trs[10 * n + 8] = trs[10 * n + 9] = 1.0f; }
    trs[10 * 34 + 0] = 0.5f; trs[10 * 34 + 1] = 0.0f;
    std::vector<uint32_t> joints(N);
    for (uint32_t n = 0; n < N; ++n) joints[n] = n;
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
    // 32 nodes at 16 sweeps (both caps); 2 nodes at 1 sweep; a two-bone goal between them; a chain that overlaps the first
    std::vector<frt_rig_goal> goals = {{FRT_GOAL_CHAIN, 1u, FRT_IK_CHAIN_MAX_SWEEPS, 32u, {0.0f, 0.0f, 0.0f}, 0u}, {FRT_GOAL_TWO_BONE, 0u, 2u, 4u, {0.0f, 0.0f, 0.0f}, 0u},
                                       {FRT_GOAL_CHAIN, 32u, 1u, 33u, {9.0f, 9.0f, 9.0f}, 0u}, {FRT_GOAL_CHAIN, 5u, 8u, 34u, {0.0f, 0.0f, 0.0f}, 0u}};
    std::vector<frt_rig_goal_target> targets = {{{9.0f, 12.0f, 5.0f}, 1.0f, {0.0f, 0.0f, 2.0f}, 1.0f}, {{1.5f, 1.0f, 0.5f}, 1.0f, {0.0f, 0.0f, 2.0f}, 1.0f},
                                                {{3.0f, 3.0f, 0.0f}, 0.5f, {0.0f, 0.0f, 0.0f}, 0.0f}, {{2.5f, 4.5f, 1.2f}, 0.75f, {0.0f, 0.0f, 0.0f}, 0.0f}};
    const uint32_t NG = (uint32_t)goals.size();
    std::vector<uint32_t> nodes = {33u, 0u, 34u};
    const float kSentinel = 7.0f;
    std::vector<float> pal(16 * N, kSentinel), mats(16 * nodes.size(), kSentinel);
    auto L = exact(layers); auto G = exact(goals); auto T = exact(targets); auto Q = exact(nodes); auto P = exact(pal); auto M = exact(mats);
    auto untouched = [&]() { for (size_t i = 0; i < pal.size(); ++i) if (P[i] != kSentinel) return false; for (size_t i = 0; i < mats.size(); ++i) if (M[i] != kSentinel) return false; return true; };
    int refusals = 0;
    auto with_goal = [&](const char* what, size_t i, frt_rig_goal g) {
        std::vector<frt_rig_goal> v = goals; v[i] = g; auto p = exact(v);
        const int a = frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, NG, p.get(), T.get(), P.get(), nullptr);
        const int b = frt_rig_evaluate_nodes_layers_ik(rig, 2u, L.get(), 0u, nullptr, NG, p.get(), T.get(), 3u, Q.get(), nullptr, nullptr, M.get());
        if (a != FRT_ERR_INVALID_ARG || b != FRT_ERR_INVALID_ARG || !untouched()) { printf("not refused, or an output written: %s\n", what); return false; }
        ++refusals;
        return true;
    };
    const bool ok = with_goal("a root out of range", 0, {FRT_GOAL_CHAIN, N, 8u, 32u, {0, 0, 0}, 0u}) && with_goal("a tip out of range", 3, {FRT_GOAL_CHAIN, 5u, 8u, N, {0, 0, 0}, 0u}) &&
                    with_goal("a tip of 2^32 - 1", 0, {FRT_GOAL_CHAIN, 1u, 8u, 0xFFFFFFFFu, {0, 0, 0}, 0u}) && with_goal("tip is root", 2, {FRT_GOAL_CHAIN, 32u, 1u, 32u, {0, 0, 0}, 0u}) &&
                    with_goal("tip above root", 2, {FRT_GOAL_CHAIN, 33u, 1u, 32u, {0, 0, 0}, 0u}) && with_goal("a tip on another branch", 3, {FRT_GOAL_CHAIN, 11u, 8u, 34u, {0, 0, 0}, 0u}) &&
                    with_goal("a path of 33 nodes", 0, {FRT_GOAL_CHAIN, 0u, 8u, 32u, {0, 0, 0}, 0u}) && with_goal("no sweeps", 0, {FRT_GOAL_CHAIN, 1u, 0u, 32u, {0, 0, 0}, 0u}) &&
                    with_goal("17 sweeps", 2, {FRT_GOAL_CHAIN, 32u, FRT_IK_CHAIN_MAX_SWEEPS + 1u, 33u, {0, 0, 0}, 0u}) && with_goal("reserved", 0, {FRT_GOAL_CHAIN, 1u, 8u, 32u, {0, 0, 0}, 31u}) &&
                    with_goal("the row of the earlier tests", 3, {2u, 0u, 0u, 0u, {0, 0, 1.0f}, 0u}) && with_goal("an unknown kind", 3, {3u, 5u, 8u, 34u, {0, 0, 0}, 0u});
    if (!ok) return 1;
    // the good calls write every output, finite; weights of zero are no goals
    if (frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, NG, G.get(), T.get(), P.get(), nullptr) != FRT_OK) { printf("evaluate_layers_ik failed\n"); return 1; }
    if (frt_rig_evaluate_nodes_layers_ik(rig, 2u, L.get(), 0u, nullptr, NG, G.get(), T.get(), 3u, Q.get(), nullptr, nullptr, M.get()) != FRT_OK) { printf("evaluate_nodes_layers_ik failed\n"); return 1; }
    for (size_t i = 0; i < pal.size(); ++i) if (P[i] == kSentinel || !std::isfinite(P[i])) { printf("palette entry %zu not written or not finite\n", i); return 1; }
    for (size_t i = 0; i < mats.size(); ++i) if (M[i] == kSentinel || !std::isfinite(M[i])) { printf("matrix entry %zu not written or not finite\n", i); return 1; }
    if (memcmp(M.get(), P.get() + 16 * 33, 64) != 0 || memcmp(M.get() + 32, P.get() + 16 * 34, 64) != 0) { printf("the node form and the palette disagree\n"); return 1; }
    std::vector<float> plain(16 * N), zero(16 * N);
    std::vector<frt_rig_goal_target> z = targets;
    for (frt_rig_goal_target& t : z) t.weight = 0.0f;
    auto Z = exact(z);
    if (frt_rig_evaluate_layers(rig, 2u, L.get(), 0u, nullptr, plain.data(), nullptr) != FRT_OK ||
        frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, NG, G.get(), Z.get(), zero.data(), nullptr) != FRT_OK) { printf("a plain call failed\n"); return 1; }
    if (memcmp(plain.data(), zero.data(), plain.size() * 4) != 0) { printf("zero weights differ from the layered call\n"); return 1; }
    if (memcmp(plain.data() + 16 * 20, P.get() + 16 * 20, 64) == 0) { printf("the goals changed nothing\n"); return 1; }
    // sixteen chains of 32 nodes at 16 sweeps, the most a call takes
    std::vector<frt_rig_goal> many(FRT_MAX_RIG_GOALS, goals[0]); std::vector<frt_rig_goal_target> many_t(FRT_MAX_RIG_GOALS, targets[0]);
    auto MG = exact(many); auto MT = exact(many_t);
    if (frt_rig_evaluate_layers_ik(rig, 2u, L.get(), 0u, nullptr, FRT_MAX_RIG_GOALS, MG.get(), MT.get(), P.get(), nullptr) != FRT_OK) { printf("sixteen chains failed\n"); return 1; }
    frt_rig_destroy(rig);
    printf("ok: %d refusals with the outputs untouched, both evaluations under chains of 2 and 32 nodes with exactly sized arrays\n", refusals);
    return 0;
}
