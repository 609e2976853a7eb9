// rig_nodes_sanitize.cpp — frt_rig_create_ex and frt_rig_evaluate_nodes (csrc/frt_animation.cpp; DESIGN.md §11, "Node animation") take counts and
// node numbers a caller controls. This stand-alone program builds nodes-only rigs and rigs with joints of the shapes the tests use (chains, a fan,
// random trees up to 1024 nodes and one beyond), evaluates node lists of 1, 9 and 300 entries with and without root and offsets at times before, at,
// between and behind the keys, and hands both functions every description and argument they have to refuse. Built host-only together with
// frt_animation.cpp under -fsanitize=address,undefined; a clean run prints "ok" and exits 0.
//   hipcc -O1 -g -std=c++17 --cuda-host-only -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -x hip tools/rig_nodes_sanitize.cpp fast-raytracing-wgpu_amd/csrc/frt_animation.cpp -o tools/_build/rig_nodes_sanitize && tools/_build/rig_nodes_sanitize
#include "../include/frt.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
namespace frt { int set_error(int code, const std::string& msg) { g_err = msg; return code; } }

struct Built {
    std::vector<int32_t> parents; std::vector<float> trs; std::vector<uint32_t> joints;
    std::vector<std::vector<float>> times, values; std::vector<frt_rig_channel> channels; frt_rig_clip clips[2]; frt_rig_desc d;
};
// kind 0: a chain, 1: a fan, 2: a random tree. `joints`: every second node is a joint; else the description has neither joints nor targets.
static void build(Built& b, uint32_t n, int kind, bool joints, std::mt19937& rng) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    b.parents.resize(n); b.trs.resize((size_t)10 * n);
    for (uint32_t i = 0; i < n; ++i) {
        b.parents[i] = i == 0 ? -1 : kind == 0 ? (int32_t)i - 1 : kind == 1 ? 0 : (int32_t)(rng() % i);
        float* p = &b.trs[(size_t)10 * i];
        for (int k = 0; k < 10; ++k) p[k] = k < 3 ? 0.3f * u(rng) : k < 7 ? u(rng) : 1.0f + 0.05f * u(rng);
    }
    if (joints) for (uint32_t i = 0; i < n; i += 2) b.joints.push_back(n - 1 - i);
    const uint32_t keys[4] = {1, 2, 5, 33};
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t path = 0; path < 3; ++path, ++c) {
            if (rng() & 1u) continue;
            const uint32_t K = keys[(c / 3) % 4], interp = c % 3, width = path == 1 ? 4u : 3u;
            std::vector<float> t(K), v((size_t)K * width * (interp == 2 ? 3 : 1));
            for (uint32_t k = 0; k < K; ++k) t[k] = 0.25f + 0.125f * (float)k;
            for (float& x : v) x = u(rng);
            b.times.push_back(t); b.values.push_back(v);
            b.channels.push_back(frt_rig_channel{i, path, interp, K, nullptr, nullptr});
        }
    for (size_t k = 0; k < b.channels.size(); ++k) { b.channels[k].times = b.times[k].data(); b.channels[k].values = b.values[k].data(); }
    b.clips[0] = frt_rig_clip{"move", (uint32_t)b.channels.size(), b.channels.data()};
    b.clips[1] = frt_rig_clip{nullptr, 0, nullptr};
    b.d = frt_rig_desc{n, b.parents.data(), b.trs.data(), nullptr, nullptr, (uint32_t)b.joints.size(), b.joints.empty() ? nullptr : b.joints.data(), nullptr, 0, nullptr, 2, b.clips};
}
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "rig_nodes_sanitize: %s failed (line %d): %s\n", #x, __LINE__, g_err.c_str()); return 1; } } while (0)

int main() {
    std::mt19937 rng(7);
    const struct { uint32_t n; int kind; bool joints; } shapes[] = {{1, 0, false}, {2, 0, true}, {70, 0, false}, {66, 1, false}, {257, 2, true}, {1024, 2, false}, {1025, 0, false}};
    size_t evaluated = 0;
    for (const auto& s : shapes) {
        Built b; build(b, s.n, s.kind, s.joints, rng);
        if (!s.joints) REQUIRE(frt_rig_create(&b.d) == nullptr && frt_rig_create_ex(&b.d, 0u) == nullptr);      // without the flag: refused as ever
        REQUIRE(frt_rig_create_ex(&b.d, 2u) == nullptr && frt_rig_create_ex(&b.d, FRT_RIG_NODES_ONLY | 4u) == nullptr);      // unknown flag bits
        frt_rig* rig = frt_rig_create_ex(&b.d, FRT_RIG_NODES_ONLY);
        REQUIRE(rig);
        uint32_t counts[4];
        REQUIRE(frt_rig_counts(rig, counts) == FRT_OK && counts[0] == s.n && counts[1] == b.joints.size() && counts[2] == 0 && counts[3] == 2);
        float root[16] = {0.5f, 0, 0, 0, 0, 0.5f, 0, 0, 0, 0, 0.5f, 0, 1, 2, 3, 1};
        for (uint32_t n : {1u, 9u, 300u}) {
            std::vector<uint32_t> nodes(n);
            for (uint32_t& x : nodes) x = rng() % s.n;
            nodes[0] = s.n - 1;      // the last node the caller named
            std::vector<float> off((size_t)16 * n, 0.0f), out((size_t)16 * n);
            for (uint32_t k = 0; k < n; ++k) off[(size_t)16 * k] = off[(size_t)16 * k + 5] = off[(size_t)16 * k + 10] = off[(size_t)16 * k + 15] = 1.0f;
            for (float t : {-1.0f, 0.25f, 0.3f, 0.375f, 4.25f, 3.0e38f})
                for (uint32_t clip = 0; clip < 2; ++clip)
                    for (int form = 0; form < 4; ++form, ++evaluated)
                        REQUIRE(frt_rig_evaluate_nodes(rig, clip, t, n, nodes.data(), form & 1 ? root : nullptr, form & 2 ? off.data() : nullptr, out.data()) == FRT_OK);
            // every argument that has to be refused
            REQUIRE(frt_rig_evaluate_nodes(rig, 2, 0.0f, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, NAN, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, -INFINITY, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, 0, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nodes.data(), nullptr, nullptr, nullptr) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nullptr, nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes(nullptr, 0, 0.3f, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            nodes[n - 1] = s.n;      // a node that is not a node
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            nodes[n - 1] = 0xFFFFFFFFu;
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nodes.data(), nullptr, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
            nodes[n - 1] = 0;
            off[(size_t)16 * n - 1] = INFINITY;
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nodes.data(), nullptr, off.data(), out.data()) == FRT_ERR_INVALID_ARG);
            float bad_root[16];
            memcpy(bad_root, root, sizeof(root));
            bad_root[15] = NAN;
            REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.3f, n, nodes.data(), bad_root, nullptr, out.data()) == FRT_ERR_INVALID_ARG);
        }
        frt_rig_destroy(rig);
    }
    // a rig without clips is created and has no clip 0
    {
        Built b; build(b, 3, 0, false, rng);
        b.d.nclips = 0; b.d.clips = nullptr;
        frt_rig* rig = frt_rig_create_ex(&b.d, FRT_RIG_NODES_ONLY);
        REQUIRE(rig);
        uint32_t node = 0; float out[16];
        REQUIRE(frt_rig_evaluate_nodes(rig, 0, 0.0f, 1, &node, nullptr, nullptr, out) == FRT_ERR_INVALID_ARG);
        frt_rig_destroy(rig);
    }
    // the descriptions frt_rig_create refuses are refused under the flag too, each a change of one thing in a good description
    int refused = 0;
    for (int bad = 0; bad < 12; ++bad) {
        Built b; build(b, 12, 2, bad & 1, rng);
        const size_t chan = b.channels.size();
        uint8_t has[12] = {};
        std::vector<float> mats((size_t)16 * 12, 0.0f);
        uint32_t bad_joint[2] = {3, 12};
        switch (bad) {
        case 0: b.d.nnodes = 0; break;
        case 1: b.parents[3] = 3; break;                          // a cycle
        case 2: b.parents[2] = 7; break;                          // a later parent
        case 3: b.parents[5] = -2; break;
        case 4: b.d.njoints = 2; b.d.joint_nodes = bad_joint; break;      // a joint that is not a node
        case 5: b.d.ntargets = FRT_MAX_MORPH_TARGETS + 1u; break;
        case 6: b.channels[0].node = 12; break;
        case 7: b.channels[0].path = FRT_RIG_PATH_WEIGHTS; break;      // a weights channel in a rig without targets
        case 8: b.channels[0].interpolation = 3; break;
        case 9: b.channels[0].nkeys = 0; break;
        case 10: b.values[chan - 1][0] = NAN; break;
        case 11: has[b.channels[0].node] = 1; b.d.has_matrix = has; b.d.matrices = mats.data(); break;      // a channel on a matrix node
        }
        frt_rig* rig = frt_rig_create_ex(&b.d, FRT_RIG_NODES_ONLY);
        if (rig) { std::fprintf(stderr, "rig_nodes_sanitize: bad description %d was accepted\n", bad); frt_rig_destroy(rig); return 1; }
        ++refused;
    }
    REQUIRE(frt_rig_create_ex(nullptr, FRT_RIG_NODES_ONLY) == nullptr);
    std::printf("ok: %zu rigs, %zu evaluations, %d descriptions refused\n", sizeof(shapes) / sizeof(shapes[0]), evaluated, refused);
    return 0;
}
