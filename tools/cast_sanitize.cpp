// cast_sanitize.cpp — the host-only half of frt_renderer_animate_cast (csrc/frt_animation.cpp: check_cast_entries, cast_layout; DESIGN.md §11,
// "Animating a cast") takes counts and binding numbers a caller controls. This stand-alone program describes lists of bindings of both kinds (1 to 300
// ids each, some unbound), hands the checks casts of 1 to FRT_MAX_CAST_ENTRIES entries in shuffled order and every call they have to refuse, and
// walks every slice of the layout of each accepted cast: the slices lie inside their sections, in order, and do not overlap. Built host-only together
// with frt_animation.cpp under -fsanitize=address,undefined; a clean run prints "ok" and exits 0.
//   hipcc -O1 -g -std=c++17 --cuda-host-only -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -x hip tools/cast_sanitize.cpp fast-raytracing-wgpu_amd/csrc/frt_animation.cpp -o tools/_build/cast_sanitize && tools/_build/cast_sanitize
#include "../include/frt.h"
#include "../fast-raytracing-wgpu_amd/csrc/frt_animation.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
namespace frt { int set_error(int code, const std::string& msg) { g_err = msg; return code; } }
using namespace frt;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "cast_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

struct World {
    std::vector<std::vector<uint32_t>> ids;      // per binding
    std::vector<CastBinding> b;
    size_t nmeshes = 0, ninstances = 0;
};
// `nb` bindings, alternately of meshes and of instances, binding k with 1 + (7 k) % 300 ids, all ids distinct within a kind; every fifth one unbound.
static void build(World& w, uint32_t nb, std::mt19937& rng) {
    w.ids.resize(nb); w.b.resize(nb);
    uint32_t next[2] = {0, 0};
    for (uint32_t k = 0; k < nb; ++k) {
        const uint32_t kind = k & 1u, n = 1u + (7u * k) % 300u;
        for (uint32_t i = 0; i < n; ++i) w.ids[k].push_back(next[kind]++);
        std::shuffle(w.ids[k].begin(), w.ids[k].end(), rng);
        CastBinding& b = w.b[k];
        b.live = k % 5u != 4u; b.kind = kind; b.nclips = 1u + k % 3u; b.njoints = kind ? 0u : (k % 4u) * 17u; b.ntargets = kind ? 0u : (k % 3u);
        b.n = n;
    }
    for (uint32_t k = 0; k < nb; ++k) w.b[k].ids = w.ids[k].data();      // (the vectors no longer move)
    w.nmeshes = next[0]; w.ninstances = next[1];
}
static std::string check(const World& w, const std::vector<frt_cast_entry>& e, uint32_t flags = 0) {
    return check_cast_entries((uint32_t)e.size(), e.data(), flags, FRT_DEFORM_RECOMPUTE_NORMALS, w.b.data(), w.b.size(), w.nmeshes, w.ninstances);
}

int main() {
    std::mt19937 rng(11);
    size_t accepted = 0, refused = 0, slices = 0;
    for (uint32_t nb : {1u, 2u, 7u, 64u, 5200u}) {
        World w; build(w, nb, rng);
        std::vector<uint32_t> live;
        for (uint32_t k = 0; k < nb; ++k) if (w.b[k].live) live.push_back(k);
        std::shuffle(live.begin(), live.end(), rng);
        for (size_t n : {(size_t)1, live.size() / 2, live.size()}) {
            n = std::min<size_t>(std::max<size_t>(n, 1), FRT_MAX_CAST_ENTRIES);
            std::vector<frt_cast_entry> e;
            for (size_t k = 0; k < n; ++k) e.push_back(frt_cast_entry{live[k], w.b[live[k]].nclips - 1u, 0.25f * (float)k, 0u});
            REQUIRE(check(w, e).empty() && check(w, e, FRT_DEFORM_RECOMPUTE_NORMALS).empty());
            ++accepted;
            const CastLayout l = cast_layout((uint32_t)e.size(), e.data(), w.b.data());
            REQUIRE(l.ids_off == 0 && l.mats_off >= (size_t)l.ninst * 4 && l.pal_off >= l.mats_off + (size_t)l.ninst * 64 && l.wt_off >= l.pal_off + (size_t)l.cols * 16 &&
                    l.bytes >= l.wt_off + (size_t)l.nweights * 4 && l.mats_off % 16 == 0 && l.pal_off % 16 == 0 && l.wt_off % 16 == 0 && l.bytes % 16 == 0);
            uint32_t inst = 0, cols = 0, weights = 0, mesh_entries = 0;
            for (size_t k = 0; k < e.size(); ++k, ++slices) {      // the slices follow each other in entry order
                const CastBinding& b = w.b[e[k].binding];
                if (b.kind) { REQUIRE(l.first[k] == inst); inst += b.n; }
                else { REQUIRE(l.first[k] == cols && l.first_weight[k] == weights); cols += 4u * b.njoints; weights += b.ntargets; ++mesh_entries; }
            }
            REQUIRE(inst == l.ninst && cols == l.cols && weights == l.nweights && mesh_entries == l.nmesh_entries);
            // every call that has to be refused: one change to the accepted cast
            std::vector<std::vector<frt_cast_entry>> bad;
            auto with = [&](size_t k, frt_cast_entry x) { std::vector<frt_cast_entry> c = e; c[k] = x; bad.push_back(c); };
            const size_t k = e.size() - 1;
            with(k, frt_cast_entry{e[k].binding, e[k].clip, e[k].time, 1u});                          // reserved
            with(k, frt_cast_entry{nb, e[k].clip, e[k].time, 0u});                                    // an unknown binding
            with(k, frt_cast_entry{0xFFFFFFFFu, e[k].clip, e[k].time, 0u});
            with(k, frt_cast_entry{e[k].binding, w.b[e[k].binding].nclips, e[k].time, 0u});          // clip out of range
            with(k, frt_cast_entry{e[k].binding, e[k].clip, NAN, 0u});                                // a time that is not finite
            with(k, frt_cast_entry{e[k].binding, e[k].clip, INFINITY, 0u});
            with(k, frt_cast_entry{e[k].binding, e[k].clip, -INFINITY, 0u});
            if (nb >= 5) with(k, frt_cast_entry{4u, 0u, 0.0f, 0u});                                   // an unbound binding
            if (e.size() >= 2) with(k, e[0]);                                                         // a binding named twice
            for (const auto& c : bad) { REQUIRE(!check(w, c).empty()); ++refused; }
            REQUIRE(!check(w, e, 2u).empty() && !check(w, e, 4u).empty());                            // unknown flag bits
            REQUIRE(!check_cast_entries(0, e.data(), 0, 1u, w.b.data(), w.b.size(), w.nmeshes, w.ninstances).empty());
            REQUIRE(!check_cast_entries((uint32_t)e.size(), nullptr, 0, 1u, w.b.data(), w.b.size(), w.nmeshes, w.ninstances).empty());
            REQUIRE(!check_cast_entries(1, e.data(), 0, 1u, nullptr, 0, w.nmeshes, w.ninstances).empty());
            refused += 5;
        }
        // more entries than FRT_MAX_CAST_ENTRIES: refused by the count, before any entry is read
        std::vector<frt_cast_entry> one(1, frt_cast_entry{live[0], 0u, 0.0f, 0u});
        REQUIRE(!check_cast_entries(FRT_MAX_CAST_ENTRIES + 1u, one.data(), 0, 1u, w.b.data(), w.b.size(), w.nmeshes, w.ninstances).empty());
        ++refused;
        // two bindings of one kind that share an id, and an id past the scene's count
        if (live.size() >= 3) {
            uint32_t a = live[0], c = 0xFFFFFFFFu;
            for (uint32_t x : live) if (x != a && w.b[x].kind == w.b[a].kind) { c = x; break; }
            if (c != 0xFFFFFFFFu) {
                const uint32_t kept = w.ids[c][w.ids[c].size() - 1];
                w.ids[c][w.ids[c].size() - 1] = w.ids[a][0];
                std::vector<frt_cast_entry> e{frt_cast_entry{a, 0u, 0.0f, 0u}, frt_cast_entry{c, 0u, 0.0f, 0u}};
                REQUIRE(check(w, e).find("two entries") != std::string::npos);
                w.ids[c][w.ids[c].size() - 1] = 0x7FFFFFFFu;
                REQUIRE(check(w, e).find("out of range") != std::string::npos);
                w.ids[c][w.ids[c].size() - 1] = kept;
                REQUIRE(check(w, e).empty());
                refused += 2;
            }
        }
    }
    std::printf("ok: %zu casts accepted, %zu slices walked, %zu calls refused\n", accepted, slices, refused);
    return 0;
}
