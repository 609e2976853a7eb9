// layers_sanitize.cpp — frt_rig_evaluate_layers, frt_rig_evaluate_nodes_layers and the host-only checks of frt_renderer_animate_cast_layers
// (csrc/frt_animation.cpp: check_clip_layers, check_rig_masks, check_cast_layers_entries; DESIGN.md §11, "Layering clips") take counts, clip and mask
// numbers and layer ranges a caller controls. This stand-alone program builds rigs of the shapes the tests use with three clips each, evaluates
// stacks of 1 to FRT_MAX_LAYERS layers of every mode with exactly sized layer lists, masks and outputs, hands both calls every list and mask set they
// have to refuse — the outputs stay as they were — and hands the cast check entries whose layer range overruns `nlayers`. Built host-only together
// with frt_animation.cpp under -fsanitize=address,undefined; a clean run prints "ok" and exits 0.
//   hipcc -O1 -g -std=c++17 --cuda-host-only -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -x hip tools/layers_sanitize.cpp fast-raytracing-wgpu_amd/csrc/frt_animation.cpp -o tools/_build/layers_sanitize && tools/_build/layers_sanitize
#include "../include/frt.h"
#include "../fast-raytracing-wgpu_amd/csrc/frt_animation.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
namespace frt { int set_error(int code, const std::string& msg) { g_err = msg; return code; } }
using namespace frt;

static const uint32_t kClips = 3;
static const uint32_t kNone = FRT_LAYER_NO_MASK;
struct Built {
    std::vector<int32_t> parents; std::vector<float> trs; std::vector<uint32_t> joints; std::vector<float> defw;
    std::vector<std::vector<float>> times, values; std::vector<frt_rig_channel> channels; uint32_t first[kClips + 1]; frt_rig_clip clips[kClips]; frt_rig_desc d;
};
// kind 0: a chain, 1: a fan, 2: a random tree. Every clip has channels on about half the node paths, every interpolation, 1 to 33 keys; the first two
// clips have a weights channel, the last takes the defaults.
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
    for (uint32_t clip = 0; clip < kClips; ++clip) {
        b.first[clip] = (uint32_t)b.channels.size();
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t path = 0; path < 3; ++path, ++c) {
                if ((rng() & 1u) && !(i == 0 && path == 0)) continue;      // (node 0's translation always: no clip is empty)
                const uint32_t K = keys[(c / 3) % 4], interp = c % 3, width = path == 1 ? 4u : 3u;
                std::vector<float> t(K), v((size_t)K * width * (interp == 2 ? 3 : 1));
                for (uint32_t k = 0; k < K; ++k) t[k] = 0.25f + 0.125f * (float)k;
                for (float& x : v) x = u(rng);
                b.times.push_back(t); b.values.push_back(v);
                b.channels.push_back(frt_rig_channel{i, path, interp, K, nullptr, nullptr});
            }
        if (ntargets && clip + 1 < kClips) {
            std::vector<float> t(33), v((size_t)33 * ntargets * 3);
            for (uint32_t k = 0; k < 33; ++k) t[k] = 0.125f * (float)k;
            for (float& x : v) x = u(rng);
            b.times.push_back(t); b.values.push_back(v);
            b.channels.push_back(frt_rig_channel{0, FRT_RIG_PATH_WEIGHTS, FRT_RIG_CUBICSPLINE, 33, nullptr, nullptr});
        }
    }
    b.first[kClips] = (uint32_t)b.channels.size();
    for (size_t k = 0; k < b.channels.size(); ++k) { b.channels[k].times = b.times[k].data(); b.channels[k].values = b.values[k].data(); }
    for (uint32_t clip = 0; clip < kClips; ++clip) b.clips[clip] = frt_rig_clip{"clip", b.first[clip + 1] - b.first[clip], b.channels.data() + b.first[clip]};
    b.d = frt_rig_desc{n, b.parents.data(), b.trs.data(), nullptr, nullptr, (uint32_t)b.joints.size(), b.joints.data(), nullptr, ntargets, ntargets ? b.defw.data() : nullptr, kClips, b.clips};
}
#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "layers_sanitize: %s failed (line %d): %s\n", #x, __LINE__, g_err.c_str()); return 1; } } while (0)

int main() {
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const float when[] = {-1.0f, 0.25f, 0.3f, 0.375f, 1.0f, 4.24f, 4.25f, 99.0f, 3.0e38f};
    size_t stacks = 0, refused = 0;
    const struct { uint32_t n; int kind; uint32_t targets; } shapes[] = {{1, 0, 3}, {2, 0, 0}, {70, 0, 3}, {66, 1, 1}, {257, 2, 3}, {1024, 2, 64}};
    for (const auto& s : shapes) {
        Built b; build(b, s.n, s.kind, s.targets, rng);
        frt_rig* rig = frt_rig_create(&b.d);
        REQUIRE(rig);
        uint32_t counts[4];
        REQUIRE(frt_rig_counts(rig, counts) == FRT_OK && counts[0] == s.n && counts[3] == kClips);
        const uint32_t nn = s.n < 40u ? s.n : 40u;
        std::vector<uint32_t> nodes(nn);
        for (uint32_t& x : nodes) x = rng() % s.n;
        std::vector<float> root(16, 0.0f), offsets((size_t)16 * nn, 0.0f);
        for (int i = 0; i < 4; ++i) root[(size_t)5 * i] = 1.0f;
        for (uint32_t k = 0; k < nn; ++k) for (int i = 0; i < 4; ++i) offsets[(size_t)16 * k + 5 * i] = 0.5f;
        // exactly sized outputs: a write past a palette, a weight vector or a matrix list is a heap overflow
        std::vector<float> pal((size_t)16 * counts[1]), w(counts[2]), ref_pal(pal.size()), ref_w(w.size()), mats((size_t)16 * nn);
        for (uint32_t n = 1; n <= FRT_MAX_LAYERS; ++n)
            for (uint32_t nmasks : {0u, 1u, 3u, FRT_MAX_RIG_MASKS})
                for (int round = 0; round < 3; ++round, ++stacks) {
                    std::vector<float> masks((size_t)nmasks * s.n);      // exactly nmasks x nnodes: a read of mask `nmasks` is a heap overflow
                    for (float& x : masks) { const uint32_t k = rng() % 4; x = k == 0 ? 0.0f : k == 1 ? 1.0f : u(rng); }
                    std::vector<frt_clip_layer> list(n);                 // exactly n: a read past the count is a heap overflow
                    list[0] = frt_clip_layer{(uint32_t)(rng() % kClips), when[rng() % 9], 0.1f + 3.0f * u(rng), kNone, FRT_LAYER_BLEND, 0u, 0.0f, 0u};
                    for (uint32_t i = 1; i < n; ++i) {
                        const uint32_t mode = rng() % 3;
                        const float weight = rng() % 4 == 0 ? 0.0f : mode == FRT_LAYER_OVERRIDE ? (rng() % 3 == 0 ? 1.0f : u(rng)) : 0.1f + 2.0f * u(rng);
                        list[i] = frt_clip_layer{(uint32_t)(rng() % kClips), when[rng() % 9], weight, nmasks && rng() % 3 ? (uint32_t)(rng() % nmasks) : kNone, mode,
                                                 mode == FRT_LAYER_ADDITIVE ? (uint32_t)(rng() % kClips) : 0u, mode == FRT_LAYER_ADDITIVE ? when[rng() % 9] : 0.0f, (uint32_t)(rng() & 1u)};
                    }
                    const float* m = nmasks ? masks.data() : nullptr;
                    REQUIRE(frt_rig_evaluate_layers(rig, n, list.data(), nmasks, m, pal.data(), w.data()) == FRT_OK);
                    REQUIRE(frt_rig_evaluate_nodes_layers(rig, n, list.data(), nmasks, m, nn, nodes.data(), nullptr, nullptr, mats.data()) == FRT_OK);
                    REQUIRE(frt_rig_evaluate_nodes_layers(rig, n, list.data(), nmasks, m, nn, nodes.data(), root.data(), offsets.data(), mats.data()) == FRT_OK);
                    // every later layer of weight 0: the base clip alone, to the bit
                    for (uint32_t i = 1; i < n; ++i) list[i].weight = 0.0f;
                    REQUIRE(frt_rig_evaluate_layers(rig, n, list.data(), nmasks, m, pal.data(), w.data()) == FRT_OK);
                    REQUIRE(frt_rig_evaluate(rig, list[0].clip, list[0].time, ref_pal.data(), ref_w.data()) == FRT_OK);
                    REQUIRE(pal.empty() || !memcmp(pal.data(), ref_pal.data(), pal.size() * 4));
                    REQUIRE(w.empty() || !memcmp(w.data(), ref_w.data(), w.size() * 4));
                }
        // the lists that have to be refused, the outputs untouched
        const frt_clip_layer base{0u, 0.3f, 1.0f, kNone, FRT_LAYER_BLEND, 0u, 0.0f, 0u};
        const frt_clip_layer over{kClips - 1u, 0.4f, 0.5f, 1u, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u};
        const frt_clip_layer add{1u, 0.4f, 1.5f, 0u, FRT_LAYER_ADDITIVE, kClips - 1u, 0.3f, FRT_LAYER_KEEP_MORPH};
        std::vector<float> masks((size_t)2 * s.n, 0.5f);
        std::vector<std::vector<frt_clip_layer>> bad;
        auto second = [&](frt_clip_layer x) { bad.push_back({base, x}); bad.push_back({base, add, x}); };
        auto first = [&](frt_clip_layer x) { bad.push_back({x}); bad.push_back({x, over}); };
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, 3u, 0u, 0.0f, 0u});                               // an unknown mode
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, 0xFFFFFFFFu, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 2u});                  // unknown flag bits
        second(frt_clip_layer{kClips, 0.3f, 0.5f, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});              // a clip out of range
        second(frt_clip_layer{0xFFFFFFFFu, 0.3f, 0.0f, 0u, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u});      // ... under a zero weight too
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_ADDITIVE, kClips, 0.0f, 0u});           // a reference clip out of range
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_BLEND, 1u, 0.0f, 0u});                  // a reference on a layer that is not additive
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_OVERRIDE, 0u, 0.5f, 0u});
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_OVERRIDE, 0u, NAN, 0u});
        second(frt_clip_layer{1u, NAN, 0.5f, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, INFINITY, 0.5f, 0u, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, -INFINITY, 0.5f, 0u, FRT_LAYER_ADDITIVE, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_ADDITIVE, 0u, NAN, 0u});
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0u, FRT_LAYER_ADDITIVE, 0u, INFINITY, 0u});
        second(frt_clip_layer{1u, 0.3f, NAN, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, 0.3f, INFINITY, 0u, FRT_LAYER_ADDITIVE, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, 0.3f, -0.5f, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});
        second(frt_clip_layer{1u, 0.3f, 1.5f, 0u, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u});               // an override weight above 1
        second(frt_clip_layer{1u, 0.3f, 0.5f, 2u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});                  // mask 2 of 2
        second(frt_clip_layer{1u, 0.3f, 0.5f, 0xFFFFFFFEu, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u});
        first(frt_clip_layer{0u, 0.3f, 1.0f, kNone, FRT_LAYER_OVERRIDE, 0u, 0.0f, 0u});             // a base that is not (BLEND, no mask, weight > 0, no flags)
        first(frt_clip_layer{0u, 0.3f, 1.0f, kNone, FRT_LAYER_ADDITIVE, 0u, 0.0f, 0u});
        first(frt_clip_layer{0u, 0.3f, 1.0f, 0u, FRT_LAYER_BLEND, 0u, 0.0f, 0u});
        first(frt_clip_layer{0u, 0.3f, 0.0f, kNone, FRT_LAYER_BLEND, 0u, 0.0f, 0u});
        first(frt_clip_layer{0u, 0.3f, 1.0f, kNone, FRT_LAYER_BLEND, 0u, 0.0f, FRT_LAYER_KEEP_MORPH});
        std::fill(pal.begin(), pal.end(), 7.0f); std::fill(w.begin(), w.end(), 7.0f); std::fill(mats.begin(), mats.end(), 7.0f);
        for (const auto& l : bad) {
            REQUIRE(frt_rig_evaluate_layers(rig, (uint32_t)l.size(), l.data(), 2, masks.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes_layers(rig, (uint32_t)l.size(), l.data(), 2, masks.data(), nn, nodes.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
            refused += 2;
        }
        const frt_clip_layer good[3] = {base, over, add};
        // the counts, before the list or the masks are read: one layer behind a count of 0, of 9 and of 2^32 - 1; one mask behind a count of 17
        for (uint32_t n : {0u, FRT_MAX_LAYERS + 1u, 0xFFFFFFFFu}) {
            std::vector<frt_clip_layer> one(1, base);
            REQUIRE(frt_rig_evaluate_layers(rig, n, one.data(), 2, masks.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes_layers(rig, n, one.data(), 2, masks.data(), nn, nodes.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
            refused += 2;
        }
        for (uint32_t nm : {FRT_MAX_RIG_MASKS + 1u, 0xFFFFFFFFu}) {
            std::vector<float> one(s.n, 1.0f);
            REQUIRE(frt_rig_evaluate_layers(rig, 1, good, nm, one.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
            REQUIRE(frt_rig_evaluate_nodes_layers(rig, 1, good, nm, one.data(), nn, nodes.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
            refused += 2;
        }
        REQUIRE(frt_rig_evaluate_layers(rig, 3, good, 1, masks.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);      // the list names mask 1 of one (masks sized for it)
        REQUIRE(frt_rig_evaluate_layers(rig, 3, good, 2, nullptr, pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        for (float x : {NAN, INFINITY, -INFINITY, -0.25f, 1.5f})
            for (size_t at : {(size_t)0, (size_t)2 * s.n - 1}) {
                std::vector<float> m2 = masks;
                m2[at] = x;
                REQUIRE(frt_rig_evaluate_layers(rig, 3, good, 2, m2.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
                REQUIRE(frt_rig_evaluate_nodes_layers(rig, 3, good, 2, m2.data(), nn, nodes.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
                refused += 2;
            }
        REQUIRE(frt_rig_evaluate_layers(rig, 3, nullptr, 2, masks.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate_layers(nullptr, 3, good, 2, masks.data(), pal.data(), w.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate_nodes_layers(rig, 3, good, 2, masks.data(), 0, nodes.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate_nodes_layers(rig, 3, good, 2, masks.data(), nn, nullptr, nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
        REQUIRE(frt_rig_evaluate_nodes_layers(rig, 3, good, 2, masks.data(), nn, nodes.data(), nullptr, nullptr, nullptr) == FRT_ERR_INVALID_ARG);
        std::vector<uint32_t> far(nodes); far[nn - 1] = s.n;
        REQUIRE(frt_rig_evaluate_nodes_layers(rig, 3, good, 2, masks.data(), nn, far.data(), nullptr, nullptr, mats.data()) == FRT_ERR_INVALID_ARG);
        refused += 8;
        for (float x : pal) REQUIRE(x == 7.0f);
        for (float x : w) REQUIRE(x == 7.0f);
        for (float x : mats) REQUIRE(x == 7.0f);
        REQUIRE(frt_rig_evaluate_layers(rig, 3, good, 2, masks.data(), pal.data(), w.data()) == FRT_OK);      // and the good list is taken
        frt_rig_destroy(rig);
    }
    // the layered cast's checks: two mesh bindings and one instance binding with 2, 0 and 1 masks, 12 layers
    const uint32_t mesh_a[2] = {0, 1}, mesh_b[1] = {2}, inst_c[3] = {0, 1, 2};
    CastBinding bind[3];
    bind[0].live = true; bind[0].kind = 0; bind[0].nclips = 3; bind[0].njoints = 5; bind[0].ntargets = 2; bind[0].ids = mesh_a; bind[0].n = 2;
    bind[1].live = true; bind[1].kind = 0; bind[1].nclips = 2; bind[1].njoints = 0; bind[1].ntargets = 4; bind[1].ids = mesh_b; bind[1].n = 1;
    bind[2].live = true; bind[2].kind = 1; bind[2].nclips = 1; bind[2].ids = inst_c; bind[2].n = 3;
    const uint32_t masks_of[3] = {2, 0, 1};
    std::vector<frt_clip_layer> layers(12);      // exactly 12: a range that overruns and is read anyway is a heap overflow
    for (uint32_t i = 0; i < 12; ++i) layers[i] = frt_clip_layer{i < 8 ? i % 2u : 0u, 0.1f * (float)i, 0.5f, kNone, FRT_LAYER_BLEND, 0u, 0.0f, 0u};
    layers[1].mask = 1u; layers[1].mode = FRT_LAYER_OVERRIDE;      // entry 1 (binding 0, two masks) only
    layers[9].mask = 0u; layers[9].mode = FRT_LAYER_ADDITIVE;      // entry 0 (binding 2, one mask) only
    std::vector<frt_cast_entry> plain;
    auto check = [&](const std::vector<frt_cast_layers_entry>& e, uint32_t nl, const frt_clip_layer* l, uint32_t flags = 0) {
        return check_cast_layers_entries((uint32_t)e.size(), e.data(), nl, l, flags, FRT_DEFORM_RECOMPUTE_NORMALS, bind, masks_of, 3, 3, 3, plain);
    };
    const std::vector<frt_cast_layers_entry> ok = {{2u, 8u, 4u, 0u}, {0u, 0u, 8u, 0u}, {1u, 4u, 2u, 0u}};      // mixed order, different counts, overlapping ranges
    REQUIRE(check(ok, 12, layers.data()).empty() && plain.size() == 3 && plain[0].binding == 2 && plain[1].clip == 0 && plain[2].clip == 0);
    const CastLayout l = cast_layout(3, plain.data(), bind);
    REQUIRE(l.ninst == 3 && l.cols == 20 && l.nweights == 6 && l.nmesh_entries == 2);
    std::vector<std::vector<frt_cast_layers_entry>> bad;
    auto with = [&](size_t k, frt_cast_layers_entry x) { std::vector<frt_cast_layers_entry> c = ok; c[k] = x; bad.push_back(c); };
    with(0, {2u, 9u, 4u, 0u});                   // one past nlayers
    with(0, {2u, 12u, 1u, 0u});                  // begins at nlayers
    with(0, {2u, 0xFFFFFFFFu, 2u, 0u});          // first + count wraps
    with(1, {0u, 11u, 8u, 0u});
    with(1, {0u, 0u, 9u, 0u});                   // more than FRT_MAX_LAYERS
    with(1, {0u, 0u, 0u, 0u});                   // an empty range
    with(1, {0u, 0u, 0xFFFFFFFFu, 0u});
    with(2, {1u, 4u, 2u, 1u});                   // reserved
    with(2, {3u, 4u, 2u, 0u});                   // an unknown binding
    with(2, {0u, 4u, 2u, 0u});                   // a binding named twice
    with(0, {2u, 0u, 2u, 0u});                   // layer 1 names clip 1 of a rig with one clip (and mask 1 of one)
    with(2, {1u, 0u, 2u, 0u});                   // layer 1 names a mask and binding 1 has none
    with(2, {1u, 9u, 2u, 0u});                   // the range's base is the additive layer
    for (const auto& c : bad) { REQUIRE(!check(c, 12, layers.data()).empty()); ++refused; }
    REQUIRE(!check(ok, 11, layers.data()).empty());      // the same entries over one layer less
    REQUIRE(!check(ok, 0, layers.data()).empty() && !check(ok, 12, nullptr).empty() && !check(ok, 12, layers.data(), 2u).empty());
    REQUIRE(!check_cast_layers_entries(0, ok.data(), 12, layers.data(), 0, 1u, bind, masks_of, 3, 3, 3, plain).empty());
    REQUIRE(!check_cast_layers_entries(3, nullptr, 12, layers.data(), 0, 1u, bind, masks_of, 3, 3, 3, plain).empty());
    REQUIRE(!check_cast_layers_entries(FRT_MAX_CAST_ENTRIES + 1u, ok.data(), 12, layers.data(), 0, 1u, bind, masks_of, 3, 3, 3, plain).empty());
    refused += 7;
    for (float bad_w : {-1.0f, NAN, INFINITY}) {
        std::vector<frt_clip_layer> l2 = layers;
        l2[3].weight = bad_w;      // inside entry 1's range only
        REQUIRE(check(ok, 12, l2.data()).find("entry 1") != std::string::npos);
        ++refused;
    }
    {
        std::vector<frt_clip_layer> l2 = layers;
        l2[8].weight = 0.0f;       // entry 0's base has no weight
        REQUIRE(check(ok, 12, l2.data()).find("entry 0") != std::string::npos);
        l2 = layers;
        l2[9].mask = 1u;           // binding 2 has one mask
        REQUIRE(check(ok, 12, l2.data()).find("entry 0") != std::string::npos);
        refused += 2;
    }
    std::printf("ok: %zu stacks evaluated, %zu calls refused\n", stacks, refused);
    return 0;
}
