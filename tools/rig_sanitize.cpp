// rig_sanitize.cpp — frt_rig_create and frt_rig_evaluate (csrc/frt_animation.cpp) parse sizes a caller controls. This stand-alone program builds rigs of
// the shapes the tests use (chains, a fan, random trees up to 1024 nodes, every interpolation, 1 to 33 keys), evaluates each at times before, at,
// between and behind the keys, and hands frt_rig_create the descriptions it has to refuse. Built host-only together with frt_animation.cpp under
// -fsanitize=address,undefined; a clean run prints "ok" and exits 0.
//   hipcc -O1 -g -std=c++17 --cuda-host-only -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -x hip tools/rig_sanitize.cpp fast-raytracing-wgpu_amd/csrc/frt_animation.cpp -o tools/_build/rig_sanitize && tools/_build/rig_sanitize
#include "../include/frt.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
namespace frt { int set_error(int code, const std::string& msg) { g_err = msg; return code; } }

struct Built {
    std::vector<int32_t> parents; std::vector<float> trs; std::vector<uint32_t> joints; std::vector<float> defw;
    std::vector<std::vector<float>> times, values; std::vector<frt_rig_channel> channels; frt_rig_clip clips[2]; frt_rig_desc d;
};
static void build(Built& b, uint32_t n, int kind, uint32_t ntargets, std::mt19937& rng) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    b.parents.resize(n); b.trs.resize((size_t)10 * n);
    for (uint32_t i = 0; i < n; ++i) {
        b.parents[i] = i == 0 ? -1 : kind == 0 ? (int32_t)i - 1 : kind == 1 ? 0 : (int32_t)(rng() % i);
        float* p = &b.trs[(size_t)10 * i];
        for (int k = 0; k < 10; ++k) p[k] = k < 3 ? 0.3f * u(rng) : k < 7 ? u(rng) : 1.0f + 0.05f * u(rng);
    }
    for (uint32_t i = 0; i < n; i += 2) b.joints.push_back(n - 1 - i);
    b.defw.assign(ntargets, 0.25f);
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
    if (ntargets) {
        std::vector<float> t(33), v((size_t)33 * ntargets * 3);
        for (uint32_t k = 0; k < 33; ++k) t[k] = 0.125f * (float)k;
        for (float& x : v) x = u(rng);
        b.times.push_back(t); b.values.push_back(v);
        b.channels.push_back(frt_rig_channel{0, FRT_RIG_PATH_WEIGHTS, FRT_RIG_CUBICSPLINE, 33, nullptr, nullptr});
    }
    for (size_t k = 0; k < b.channels.size(); ++k) { b.channels[k].times = b.times[k].data(); b.channels[k].values = b.values[k].data(); }
    b.clips[0] = frt_rig_clip{"move", (uint32_t)b.channels.size(), b.channels.data()};
    b.clips[1] = frt_rig_clip{nullptr, 0, nullptr};
    b.d = frt_rig_desc{n, b.parents.data(), b.trs.data(), nullptr, nullptr, (uint32_t)b.joints.size(), b.joints.data(), nullptr, ntargets, ntargets ? b.defw.data() : nullptr, 2, b.clips};
}
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "rig_sanitize: %s failed (line %d): %s\n", #x, __LINE__, g_err.c_str()); return 1; } } while (0)

int main() {
    std::mt19937 rng(7);
    const struct { uint32_t n; int kind; uint32_t targets; } shapes[] = {{1, 0, 3}, {2, 0, 0}, {70, 0, 3}, {66, 1, 1}, {257, 2, 3}, {1024, 2, 4096}, {1025, 0, 0}};
    for (const auto& s : shapes) {
        Built b; build(b, s.n, s.kind, s.targets, rng);
        frt_rig* rig = frt_rig_create(&b.d);
        REQUIRE(rig);
        uint32_t counts[4];
        REQUIRE(frt_rig_counts(rig, counts) == FRT_OK && counts[0] == s.n && counts[3] == 2);
        std::vector<float> pal((size_t)16 * counts[1]), w(counts[2]);
        for (float t : {-1.0f, 0.25f, 0.3f, 0.375f, 1.0f, 4.24f, 4.25f, 99.0f, 3.0e38f})
            for (uint32_t clip = 0; clip < 2; ++clip) REQUIRE(frt_rig_evaluate(rig, clip, t, pal.data(), w.data()) == FRT_OK);
        REQUIRE(frt_rig_evaluate(rig, 2, 0.0f, pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate(rig, 0, NAN, pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate(rig, 0, INFINITY, pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        const char* name = nullptr; float dur = 0.0f;
        REQUIRE(frt_rig_clip_info(rig, 0, &name, &dur) == FRT_OK && name && frt_rig_clip_info(rig, 2, &name, &dur) == FRT_ERR_INVALID_ARG);
        frt_rig_destroy(rig);
    }
    // what has to be refused, each a change of one thing in a good description
    int refused = 0;
    for (int bad = 0; bad < 14; ++bad) {
        Built b; build(b, 12, 2, 3, rng);
        const size_t chan = b.channels.size();
        float nanv = NAN;
        uint8_t has[12] = {};
        switch (bad) {
        case 0: b.d.nnodes = 0; break;
        case 1: b.parents[3] = 3; break;                          // a cycle
        case 2: b.parents[2] = 7; break;                          // a later parent
        case 3: b.parents[5] = -2; break;
        case 4: b.joints[1] = 12; break;                          // a joint that is not a node
        case 5: b.d.njoints = 0; b.d.ntargets = 0; b.clips[0].nchannels = (uint32_t)chan - 1; break;
        case 6: b.d.ntargets = FRT_MAX_MORPH_TARGETS + 1u; break;
        case 7: b.channels[0].node = 12; break;
        case 8: b.channels[0].path = 4; break;
        case 9: b.channels[0].interpolation = 3; break;
        case 10: b.channels[0].nkeys = 0; break;
        case 11: b.times[chan - 1][7] = b.times[chan - 1][6]; break;      // key times that do not increase
        case 12: b.values[chan - 1][5] = nanv; break;
        case 13: has[b.channels[0].node] = 1; b.d.has_matrix = has; b.d.matrices = b.trs.data(); break;      // a channel on a matrix node (matrices: any 16 n floats)
        }
        std::vector<float> mats((size_t)16 * 12, 0.0f);
        if (bad == 13) b.d.matrices = mats.data();
        frt_rig* rig = frt_rig_create(&b.d);
        if (rig) { std::fprintf(stderr, "rig_sanitize: bad description %d was accepted\n", bad); frt_rig_destroy(rig); return 1; }
        ++refused;
    }
    REQUIRE(frt_rig_create(nullptr) == nullptr);
    std::printf("ok: %zu rigs evaluated, %d descriptions refused\n", sizeof(shapes) / sizeof(shapes[0]), refused);
    return 0;
}
