// frt_animation.cpp — the host form of an animated rig (include/frt.h: frt_rig_*; DESIGN.md §11, "Animation"): frt_rig_create checks a description and
// packs it into the one block frt_animation.hpp reads; frt_rig_evaluate is the specification of frt_renderer_animate's kernel, the same FRT_HD functions
// run node by node in the block's order (parents first); frt_rig_evaluate_blend and frt_rig_evaluate_nodes_blend ("Blending clips") are the same for
// a list of samples, frt_rig_evaluate_layers and frt_rig_evaluate_nodes_layers ("Layering clips") for a list of layers under masks. Host code only;
// nothing here touches a device.
#include "frt_animation.hpp"
#include "frt_loader.hpp"      // frt_model: frt_rig_from_model and the frt_model_* accessors of the rig
#include "../../include/frt.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace frt { int set_error(int code, const std::string& msg); }
using namespace frt;

static int rig_fail(const std::string& msg) { return frt::set_error(FRT_ERR_INVALID_ARG, msg); }
static bool all_finite(const float* p, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false; return true; }
static uint32_t path_width(uint32_t path, uint32_t ntargets) { return path == (uint32_t)kRigPathRotation ? 4u : path == (uint32_t)kRigPathWeights ? ntargets : 3u; }

// frt_renderer_animate_cast's entry checks and the layout of its buffer (frt_animation.hpp).
std::string frt::check_cast_entries(uint32_t n, const frt_cast_entry* e, uint32_t flags, uint32_t allowed_flags, const CastBinding* bindings, size_t nbindings,
                                    size_t nmeshes, size_t ninstances) {
    if (n == 0 || n > FRT_MAX_CAST_ENTRIES) return std::to_string(n) + " entries (1 .. FRT_MAX_CAST_ENTRIES)";
    if (!e) return "null entries";
    if (flags & ~allowed_flags) return "unknown flag bits";
    std::vector<uint8_t> named(nbindings, 0), posed(nmeshes, 0), moved(ninstances, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const std::string at = "entry " + std::to_string(k) + ": ";
        if (e[k].reserved != 0) return at + "reserved must be 0";
        if (e[k].binding >= nbindings || !bindings || !bindings[e[k].binding].live) return at + "unknown rig binding " + std::to_string(e[k].binding);
        const CastBinding& b = bindings[e[k].binding];
        if (named[e[k].binding]) return at + "binding " + std::to_string(e[k].binding) + " is named twice";
        named[e[k].binding] = 1;
        if (e[k].clip >= b.nclips) return at + "clip " + std::to_string(e[k].clip) + " out of range (" + std::to_string(b.nclips) + " clips)";
        if (!std::isfinite(e[k].time)) return at + "time is not finite";
        std::vector<uint8_t>& seen = b.kind == 0 ? posed : moved;
        if (b.n && !b.ids) return at + "a binding without ids";
        for (uint32_t i = 0; i < b.n; ++i) {
            const uint32_t id = b.ids[i];
            if (id >= seen.size()) return at + (b.kind == 0 ? "mesh id " : "instance id ") + std::to_string(id) + " out of range";
            if (seen[id]) return at + (b.kind == 0 ? "mesh " + std::to_string(id) + " is posed by two entries" : "instance " + std::to_string(id) + " is moved by two entries");
            seen[id] = 1;
        }
    }
    return "";
}
CastLayout frt::cast_layout(uint32_t n, const frt_cast_entry* e, const CastBinding* bindings) {
    CastLayout l;
    l.first.resize(n); l.first_weight.assign(n, 0u);
    for (uint32_t k = 0; k < n; ++k) {
        const CastBinding& b = bindings[e[k].binding];
        if (b.kind == 0) { l.first[k] = l.cols; l.first_weight[k] = l.nweights; l.cols += 4u * b.njoints; l.nweights += b.ntargets; ++l.nmesh_entries; }
        else { l.first[k] = l.ninst; l.ninst += b.n; }
    }
    auto put = [&l](size_t bytes) { const size_t off = l.bytes; l.bytes += (bytes + 15u) & ~(size_t)15u; return off; };
    l.ids_off = put((size_t)l.ninst * 4); l.mats_off = put((size_t)l.ninst * 64); l.pal_off = put((size_t)l.cols * 16); l.wt_off = put((size_t)l.nweights * 4);
    return l;
}

// "Blending clips": the checks of a sample list and of a blended cast (frt_animation.hpp).
std::string frt::check_blend_samples(uint32_t n, const frt_clip_sample* s, uint32_t nclips) {
    if (n == 0 || n > FRT_MAX_BLEND_SAMPLES) return std::to_string(n) + " samples (1 .. FRT_MAX_BLEND_SAMPLES)";
    if (!s) return "null samples";
    bool positive = false;
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = "sample " + std::to_string(i) + ": ";
        if (s[i].reserved != 0) return at + "reserved must be 0";
        if (s[i].clip >= nclips) return at + "clip " + std::to_string(s[i].clip) + " out of range (" + std::to_string(nclips) + " clips)";
        if (!std::isfinite(s[i].time)) return at + "time is not finite";
        if (!std::isfinite(s[i].weight)) return at + "weight is not finite";
        if (s[i].weight < 0.0f) return at + "a negative weight";
        positive = positive || s[i].weight > 0.0f;
    }
    return positive ? "" : "no sample has a positive weight";
}
std::string frt::check_cast_blend_entries(uint32_t n, const frt_cast_blend_entry* e, uint32_t nsamples, const frt_clip_sample* samples, uint32_t flags,
                                          uint32_t allowed_flags, const CastBinding* bindings, size_t nbindings, size_t nmeshes, size_t ninstances,
                                          std::vector<frt_cast_entry>& plain) {
    plain.clear();
    if (n == 0 || n > FRT_MAX_CAST_ENTRIES) return std::to_string(n) + " entries (1 .. FRT_MAX_CAST_ENTRIES)";
    if (!e) return "null entries";
    if (nsamples == 0) return "0 samples";
    if (!samples) return "null samples";
    for (uint32_t k = 0; k < n; ++k) {
        const std::string at = "entry " + std::to_string(k) + ": ";
        if (e[k].reserved != 0) return at + "reserved must be 0";
        if (e[k].num_samples == 0 || e[k].num_samples > FRT_MAX_BLEND_SAMPLES) return at + std::to_string(e[k].num_samples) + " samples (1 .. FRT_MAX_BLEND_SAMPLES)";
        if (e[k].first_sample >= nsamples || e[k].num_samples > nsamples - e[k].first_sample)
            return at + "samples " + std::to_string(e[k].first_sample) + " + " + std::to_string(e[k].num_samples) + " overrun the " + std::to_string(nsamples) + " given";
    }
    plain.resize(n);
    for (uint32_t k = 0; k < n; ++k) plain[k] = frt_cast_entry{e[k].binding, samples[e[k].first_sample].clip, samples[e[k].first_sample].time, 0u};
    const std::string bad = check_cast_entries(n, plain.data(), flags, allowed_flags, bindings, nbindings, nmeshes, ninstances);
    if (!bad.empty()) return bad;
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s = check_blend_samples(e[k].num_samples, samples + e[k].first_sample, bindings[e[k].binding].nclips);
        if (!s.empty()) return "entry " + std::to_string(k) + ": " + s;
    }
    return "";
}

// "Layering clips": the checks of a layer list, of masks where they enter and of a layered cast (frt_animation.hpp).
std::string frt::check_clip_layers(uint32_t n, const frt_clip_layer* l, uint32_t nclips, uint32_t nmasks) {
    if (n == 0 || n > FRT_MAX_LAYERS) return std::to_string(n) + " layers (1 .. FRT_MAX_LAYERS)";
    if (!l) return "null layers";
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = "layer " + std::to_string(i) + ": ";
        if (l[i].mode > (uint32_t)FRT_LAYER_ADDITIVE) return at + "unknown mode " + std::to_string(l[i].mode);
        if (l[i].flags & ~FRT_LAYER_KEEP_MORPH) return at + "unknown flag bits";
        if (l[i].clip >= nclips) return at + "clip " + std::to_string(l[i].clip) + " out of range (" + std::to_string(nclips) + " clips)";
        if (l[i].mode == (uint32_t)FRT_LAYER_ADDITIVE) {
            if (l[i].ref_clip >= nclips) return at + "reference clip " + std::to_string(l[i].ref_clip) + " out of range (" + std::to_string(nclips) + " clips)";
        } else if (l[i].ref_clip != 0 || !(l[i].ref_time == 0.0f)) return at + "ref_clip and ref_time must be 0 unless the layer is additive";
        if (!std::isfinite(l[i].time)) return at + "time is not finite";
        if (!std::isfinite(l[i].ref_time)) return at + "reference time is not finite";
        if (!std::isfinite(l[i].weight)) return at + "weight is not finite";
        if (l[i].weight < 0.0f) return at + "a negative weight";
        if (l[i].mode == (uint32_t)FRT_LAYER_OVERRIDE && l[i].weight > 1.0f) return at + "an override weight above 1";
        if (l[i].mask != FRT_LAYER_NO_MASK && l[i].mask >= nmasks) return at + "mask " + std::to_string(l[i].mask) + " out of range (" + std::to_string(nmasks) + " masks)";
    }
    if (l[0].mode != (uint32_t)FRT_LAYER_BLEND || l[0].mask != FRT_LAYER_NO_MASK || !(l[0].weight > 0.0f) || l[0].flags)
        return "layer 0 is the base: a blend layer without a mask, with a positive weight and no flags";
    return "";
}
std::string frt::check_rig_masks(uint32_t nmasks, const float* masks, uint32_t nnodes) {
    if (nmasks > FRT_MAX_RIG_MASKS) return std::to_string(nmasks) + " masks, more than FRT_MAX_RIG_MASKS";
    if (nmasks && !masks) return "null masks";
    for (size_t i = 0; i < (size_t)nmasks * nnodes; ++i)
        if (!(masks[i] >= 0.0f && masks[i] <= 1.0f)) return "mask " + std::to_string(i / nnodes) + ", node " + std::to_string(i % nnodes) + ": a mask value is a finite number in [0, 1]";
    return "";
}
// "Inverse kinematics": the pre-order numbers of the stored nodes, and the checks of goals and of host targets (frt_animation.hpp).
RigTree frt::rig_tree(const RigView& v) {
    const RigHeader h = v.h();
    const uint32_t N = h.nnodes;
    std::vector<uint32_t> size(N, 1u), next(N, 0u);
    for (uint32_t n = N; n-- > 1u;) { const uint32_t p = v.w[h.parent + n]; if (p != kRigNone) size[p] += size[n]; }      // (parents in front of their children)
    RigTree t;
    t.enter.resize(N); t.exit.resize(N);
    uint32_t roots = 0;      // the next free number among the roots
    for (uint32_t n = 0; n < N; ++n) {
        const uint32_t p = v.w[h.parent + n];
        uint32_t& at = p == kRigNone ? roots : next[p];
        t.enter[n] = at; t.exit[n] = at + size[n];
        at += size[n];
        next[n] = t.enter[n] + 1u;
    }
    return t;
}
std::string frt::check_rig_goals(uint32_t ngoals, const frt_rig_goal* goals, const std::vector<uint32_t>& place, const uint32_t* enter, const uint32_t* exit, std::vector<frt_rig_goal>& stored) {
    stored.clear();
    if (ngoals > FRT_MAX_RIG_GOALS) return std::to_string(ngoals) + " goals, more than FRT_MAX_RIG_GOALS";
    if (ngoals && !goals) return "null goals";
    const uint32_t N = (uint32_t)place.size();
    auto below = [enter, exit](uint32_t a, uint32_t d) { return a != d && ik_in_subtree(enter, exit, a, d); };      // d a strict descendant of a
    for (uint32_t i = 0; i < ngoals; ++i) {
        const frt_rig_goal& g = goals[i];
        const std::string at = "goal " + std::to_string(i) + ": ";
        if (g.kind > FRT_GOAL_CHAIN) return at + "unknown kind " + std::to_string(g.kind);
        if (g.reserved != 0) return at + "reserved must be 0";
        const bool chain = g.kind == FRT_GOAL_CHAIN;      // (its mid is a number of sweeps, not a node)
        if (g.root >= N || (!chain && g.mid >= N) || g.tip >= N) return at + "a node out of range (" + std::to_string(N) + " nodes)";
        frt_rig_goal s = g;
        if (chain) {
            s.root = place[g.root]; s.tip = place[g.tip];
            if (!below(s.root, s.tip)) return at + "the tip of a chain is not a strict descendant of its root";
            uint32_t K = 0;      // the bones of the path: the nodes of subtree(root) that hold the tip below them
            for (uint32_t a = 0; a < N; ++a) K += ik_in_subtree(enter, exit, s.root, a) && below(a, s.tip);
            if (K + 1u > FRT_IK_CHAIN_MAX_NODES) return at + "a chain of " + std::to_string(K + 1u) + " nodes, more than FRT_IK_CHAIN_MAX_NODES";
            if (g.mid < 1u || g.mid > FRT_IK_CHAIN_MAX_SWEEPS) return at + std::to_string(g.mid) + " sweeps (1 .. FRT_IK_CHAIN_MAX_SWEEPS)";
            s.axis[0] = s.axis[1] = s.axis[2] = 0.0f;      // (a chain has no axis: nothing of it is kept)
            s.reserved = K;                                // the stored form carries the path's length
        } else if (g.kind == (uint32_t)FRT_GOAL_AIM) {
            if (g.mid != 0 || g.tip != 0) return at + "mid and tip of an aim goal must be 0";
            if (!all_finite(g.axis, 3)) return at + "the axis is not finite";
            if (g.axis[0] == 0.0f && g.axis[1] == 0.0f && g.axis[2] == 0.0f) return at + "the axis is zero";
            s.root = place[g.root]; s.mid = 0u; s.tip = 0u;
        } else {
            s.root = place[g.root]; s.mid = place[g.mid]; s.tip = place[g.tip];
            if (!below(s.root, s.mid)) return at + "mid is not a strict descendant of root";
            if (!below(s.mid, s.tip)) return at + "tip is not a strict descendant of mid";
            s.axis[0] = s.axis[1] = s.axis[2] = 0.0f;      // (a two-bone goal has no axis: nothing of it is kept)
        }
        stored.push_back(s);
    }
    return "";
}
std::string frt::check_rig_goal_targets(uint32_t ngoals, const frt_rig_goal_target* targets, uint32_t bound, const frt_rig_goal* goals) {
    if (ngoals > FRT_MAX_RIG_GOALS) return std::to_string(ngoals) + " targets, more than FRT_MAX_RIG_GOALS";
    if (ngoals != bound) return std::to_string(ngoals) + " targets for " + std::to_string(bound) + " goals";
    if (ngoals && !targets) return "null targets";
    for (uint32_t i = 0; i < ngoals; ++i) {
        const frt_rig_goal_target& t = targets[i];
        const std::string at = "target " + std::to_string(i) + ": ";
        if (!all_finite(t.target, 3) || !std::isfinite(t.weight) || !all_finite(t.pole, 3) || !std::isfinite(t.pole_flag)) return at + "a word is not finite";
        if (!(t.weight >= 0.0f && t.weight <= 1.0f)) return at + "a weight lies in [0, 1]";
        if (t.pole_flag != 0.0f && t.pole_flag != 1.0f) return at + "the pole flag is 0 or 1";
        if (goals[i].kind == (uint32_t)FRT_GOAL_AIM && (t.pole_flag != 0.0f || t.pole[0] != 0.0f || t.pole[1] != 0.0f || t.pole[2] != 0.0f)) return at + "an aim goal has no pole";
    }
    return "";
}
std::string frt::check_cast_layers_entries(uint32_t n, const frt_cast_layers_entry* e, uint32_t nlayers, const frt_clip_layer* layers, uint32_t flags,
                                           uint32_t allowed_flags, const CastBinding* bindings, const uint32_t* masks_of, size_t nbindings, size_t nmeshes,
                                           size_t ninstances, std::vector<frt_cast_entry>& plain) {
    plain.clear();
    if (n == 0 || n > FRT_MAX_CAST_ENTRIES) return std::to_string(n) + " entries (1 .. FRT_MAX_CAST_ENTRIES)";
    if (!e) return "null entries";
    if (nlayers == 0) return "0 layers";
    if (!layers) return "null layers";
    for (uint32_t k = 0; k < n; ++k) {
        const std::string at = "entry " + std::to_string(k) + ": ";
        if (e[k].reserved != 0) return at + "reserved must be 0";
        if (e[k].num_layers == 0 || e[k].num_layers > FRT_MAX_LAYERS) return at + std::to_string(e[k].num_layers) + " layers (1 .. FRT_MAX_LAYERS)";
        if (e[k].first_layer >= nlayers || e[k].num_layers > nlayers - e[k].first_layer)
            return at + "layers " + std::to_string(e[k].first_layer) + " + " + std::to_string(e[k].num_layers) + " overrun the " + std::to_string(nlayers) + " given";
    }
    plain.resize(n);
    for (uint32_t k = 0; k < n; ++k) {      // (a clip or a time check_cast_entries would refuse is refused there, named as the entry's)
        const frt_clip_layer& base = layers[e[k].first_layer];
        plain[k] = frt_cast_entry{e[k].binding, base.clip, base.time, 0u};
    }
    const std::string bad = check_cast_entries(n, plain.data(), flags, allowed_flags, bindings, nbindings, nmeshes, ninstances);
    if (!bad.empty()) return bad;
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s = check_clip_layers(e[k].num_layers, layers + e[k].first_layer, bindings[e[k].binding].nclips, masks_of ? masks_of[e[k].binding] : 0u);
        if (!s.empty()) return "entry " + std::to_string(k) + ": " + s;
    }
    return "";
}

// "" or what is wrong with the description. Every count is checked before the array it sizes is read.
static std::string check_rig_desc(const frt_rig_desc* d, uint32_t flags) {
    if (!d) return "null description";
    if (d->nnodes == 0 || d->nnodes > (1u << 20)) return "nnodes must be 1 .. 2^20";
    if (!d->parents || !d->rest_trs) return "parents and rest_trs are required";
    if (d->njoints > 0x10000u) return "more than 65536 joints (a joint index is 16 bits)";
    if (d->ntargets > FRT_MAX_MORPH_TARGETS) return "more than FRT_MAX_MORPH_TARGETS targets";
    if (d->njoints == 0 && d->ntargets == 0 && !(flags & FRT_RIG_NODES_ONLY)) return "a rig has joints, morph targets or both";
    if (d->njoints && !d->joint_nodes) return "joint_nodes is required with njoints > 0";
    if (d->nclips > (1u << 16)) return "more than 65536 clips";
    if (d->nclips && !d->clips) return "clips is required with nclips > 0";
    for (uint32_t n = 0; n < d->nnodes; ++n) {
        const int32_t p = d->parents[n];
        if (p < -1 || (p >= 0 && (uint32_t)p >= n)) return "node " + std::to_string(n) + ": a parent is -1 or a smaller node index (parents first)";
        const bool mat = d->has_matrix && d->has_matrix[n];
        if (mat && !d->matrices) return "has_matrix names node " + std::to_string(n) + " but matrices is null";
        if (!(mat ? all_finite(d->matrices + (size_t)16 * n, 16) : all_finite(d->rest_trs + (size_t)10 * n, 10))) return "node " + std::to_string(n) + ": a rest value is not finite";
    }
    for (uint32_t j = 0; j < d->njoints; ++j)
        if (d->joint_nodes[j] >= d->nnodes) return "joint " + std::to_string(j) + " is not a node";
    if (d->inverse_bind && !all_finite(d->inverse_bind, (size_t)16 * d->njoints)) return "an inverse bind matrix entry is not finite";
    if (d->default_weights && !all_finite(d->default_weights, d->ntargets)) return "a default morph weight is not finite";
    uint64_t words = 0;
    for (uint32_t c = 0; c < d->nclips; ++c) {
        const frt_rig_clip& cl = d->clips[c];
        const std::string where = "clip " + std::to_string(c);
        if (cl.nchannels > (1u << 20)) return where + ": more than 2^20 channels";
        if (cl.nchannels && !cl.channels) return where + ": channels is null";
        std::vector<uint8_t> seen((size_t)3 * d->nnodes, 0);
        bool weights = false;
        for (uint32_t k = 0; k < cl.nchannels; ++k) {
            const frt_rig_channel& ch = cl.channels[k];
            const std::string at = where + ", channel " + std::to_string(k);
            if (ch.path > (uint32_t)kRigPathWeights) return at + ": unknown path";
            if (ch.interpolation > (uint32_t)kRigCubic) return at + ": unknown interpolation";
            if (ch.nkeys == 0 || ch.nkeys > (1u << 24)) return at + ": nkeys must be 1 .. 2^24";
            if (!ch.times || !ch.values) return at + ": times and values are required";
            if (ch.path == (uint32_t)kRigPathWeights) {
                if (d->ntargets == 0) return at + ": a weights channel in a rig without morph targets";
                if (weights) return at + ": a second weights channel in one clip";
                weights = true;
            } else {
                if (ch.node >= d->nnodes) return at + ": its node is not a node";
                if (d->has_matrix && d->has_matrix[ch.node]) return at + ": a node given as a matrix cannot be animated";
                uint8_t& s = seen[(size_t)3 * ch.node + ch.path];
                if (s) return at + ": a second channel for the same node and path";
                s = 1;
            }
            for (uint32_t i = 0; i < ch.nkeys; ++i)
                if (!std::isfinite(ch.times[i]) || (i && !(ch.times[i] > ch.times[i - 1]))) return at + ": key times must be finite and strictly increasing";
            const uint64_t nv = (uint64_t)ch.nkeys * path_width(ch.path, d->ntargets) * (ch.interpolation == (uint32_t)kRigCubic ? 3u : 1u);
            if (!all_finite(ch.values, (size_t)nv)) return at + ": a key value is not finite";
            words += nv + ch.nkeys + 8u;
        }
        words += (uint64_t)3 * d->nnodes + 4u;
    }
    words += (uint64_t)d->nnodes * 19u + (uint64_t)d->njoints * 17u + d->ntargets + 64u;
    if (words > (1ull << 28)) return "the rig needs more than 1 GiB";
    return "";
}

extern "C" {

frt_rig* frt_rig_create(const frt_rig_desc* d) { return frt_rig_create_ex(d, 0u); }

frt_rig* frt_rig_create_ex(const frt_rig_desc* d, uint32_t flags) {
    if (flags & ~FRT_RIG_NODES_ONLY) { rig_fail("rig_create: unknown flag bits"); return nullptr; }
    const std::string bad = check_rig_desc(d, flags);
    if (!bad.empty()) { rig_fail("rig_create: " + bad); return nullptr; }
    const uint32_t N = d->nnodes, J = d->njoints, T = d->ntargets;
    // by depth, parents in front of their children: `order[i]` is the caller's index of node i here
    std::vector<uint32_t> depth(N, 0u), order(N), place(N);
    for (uint32_t n = 0; n < N; ++n) { depth[n] = d->parents[n] < 0 ? 0u : depth[(uint32_t)d->parents[n]] + 1u; order[n] = n; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return depth[a] < depth[b]; });
    for (uint32_t i = 0; i < N; ++i) place[order[i]] = i;
    const uint32_t nlevels = depth[order[N - 1]] + 1u;
    uint32_t nchannels = 0;
    for (uint32_t c = 0; c < d->nclips; ++c) nchannels += d->clips[c].nchannels;

    frt_rig* rig = new frt_rig();
    std::vector<uint32_t>& w = rig->words;
    auto put = [&w](size_t n) { const uint32_t at = (uint32_t)w.size(); w.resize(w.size() + ((n + 3u) & ~(size_t)3u), 0u); return at; };      // (every table 16-byte aligned)
    auto fl = [&w](uint32_t at) { return reinterpret_cast<float*>(w.data() + at); };
    RigHeader h;
    memset(&h, 0, sizeof(h));
    put(sizeof(RigHeader) / 4);
    h.nnodes = N; h.njoints = J; h.ntargets = T; h.nclips = d->nclips; h.nlevels = nlevels; h.nchannels = nchannels;
    h.parent = put(N); h.kind = put(N); h.rest = put((size_t)16 * N); h.level_begin = put(nlevels + 1u);
    h.joint_node = put(J); h.inv_bind = put((size_t)16 * J); h.def_weights = put(T);
    h.clips = put((size_t)4 * d->nclips); h.channels = put((size_t)8 * nchannels);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t n = order[i];
        w[h.parent + i] = d->parents[n] < 0 ? kRigNone : place[(uint32_t)d->parents[n]];
        const bool mat = d->has_matrix && d->has_matrix[n];
        w[h.kind + i] = mat ? 1u : 0u;
        float* r = fl(h.rest) + (size_t)16 * i;
        if (mat) memcpy(r, d->matrices + (size_t)16 * n, 64);
        else { const float* s = d->rest_trs + (size_t)10 * n; memcpy(r, s, 12); memcpy(r + 4, s + 3, 16); memcpy(r + 8, s + 7, 12); }
        if (i == 0 || depth[n] != depth[order[i - 1]]) w[h.level_begin + depth[n]] = i;
    }
    w[h.level_begin + nlevels] = N;
    for (uint32_t j = 0; j < J; ++j) {
        w[h.joint_node + j] = place[d->joint_nodes[j]];
        float* m = fl(h.inv_bind) + (size_t)16 * j;
        if (d->inverse_bind) memcpy(m, d->inverse_bind + (size_t)16 * j, 64);
        else m[0] = m[5] = m[10] = m[15] = 1.0f;
    }
    if (d->default_weights && T) memcpy(fl(h.def_weights), d->default_weights, (size_t)4 * T);
    uint32_t chan = 0;
    for (uint32_t c = 0; c < d->nclips; ++c) {
        const frt_rig_clip& cl = d->clips[c];
        RigClip rc; rc.node_table = put((size_t)3 * N); rc.weights_channel = kRigNone; rc.pad0 = rc.pad1 = 0u;
        for (size_t i = 0; i < (size_t)3 * N; ++i) w[rc.node_table + i] = kRigNone;
        float duration = 0.0f;
        for (uint32_t k = 0; k < cl.nchannels; ++k, ++chan) {
            const frt_rig_channel& ch = cl.channels[k];
            RigChannel r;
            memset(&r, 0, sizeof(r));
            r.path = ch.path; r.interp = ch.interpolation; r.nkeys = ch.nkeys; r.width = path_width(ch.path, T);
            const size_t nv = (size_t)ch.nkeys * r.width * (ch.interpolation == (uint32_t)kRigCubic ? 3u : 1u);
            r.times = put(ch.nkeys); r.values = put(nv);
            memcpy(fl(r.times), ch.times, (size_t)4 * ch.nkeys);
            memcpy(fl(r.values), ch.values, 4 * nv);
            if (ch.path == (uint32_t)kRigPathWeights) { r.node = kRigNone; rc.weights_channel = chan; }
            else { r.node = place[ch.node]; w[rc.node_table + (size_t)3 * r.node + ch.path] = chan; }
            memcpy(w.data() + h.channels + (size_t)8 * chan, &r, sizeof(r));
            duration = std::max(duration, ch.times[ch.nkeys - 1]);
        }
        memcpy(w.data() + h.clips + (size_t)4 * c, &rc, sizeof(rc));
        rig->clip_names.push_back(cl.name ? cl.name : "");
        rig->clip_durations.push_back(duration);
    }
    h.words = (uint32_t)w.size();
    memcpy(w.data(), &h, sizeof(h));
    rig->place.swap(place);
    return rig;
}

void frt_rig_destroy(frt_rig* rig) { delete rig; }

// ---- the rig a loaded glTF document holds (frt_loader.cpp: read_rig): plain copies out of LoadedModel
int frt_model_rig_counts(const frt_model* m, uint32_t out[3]) {
    if (!m || !out) return rig_fail("model_rig_counts: null");
    out[0] = (uint32_t)m->m.nodes.size(); out[1] = (uint32_t)m->m.skins.size(); out[2] = (uint32_t)m->m.animations.size();
    return FRT_OK;
}
int frt_model_geometry_rig(const frt_model* m, uint32_t geo, uint32_t out[4]) {
    if (!m || !out || geo >= m->m.geometries.size()) return rig_fail("model_geometry_rig: bad arguments");
    out[0] = 0u; out[1] = kRigNone; out[2] = 0u; out[3] = kRigNone;
    if (geo >= m->m.geometry_rigs.size()) return FRT_OK;      // (an OBJ model)
    const LoadedModel::GeometryRig& g = m->m.geometry_rigs[geo];
    out[0] = g.joints.empty() ? 0u : 1u; out[1] = g.skin < 0 ? kRigNone : (uint32_t)g.skin; out[2] = g.ntargets; out[3] = g.mesh < 0 ? kRigNone : (uint32_t)g.mesh;
    return FRT_OK;
}
int frt_model_geometry_skin_get(const frt_model* m, uint32_t geo, uint16_t* joints4, float* weights4) {
    if (!m || geo >= m->m.geometry_rigs.size() || m->m.geometry_rigs[geo].joints.empty() || !joints4 || !weights4) return rig_fail("model_geometry_skin_get: bad arguments or a geometry without skin attributes");
    const LoadedModel::GeometryRig& g = m->m.geometry_rigs[geo];
    memcpy(joints4, g.joints.data(), g.joints.size() * 2); memcpy(weights4, g.weights.data(), g.weights.size() * 4);
    return FRT_OK;
}
int frt_model_geometry_targets_get(const frt_model* m, uint32_t geo, float* deltas3, float* default_weights) {
    if (!m || geo >= m->m.geometry_rigs.size() || m->m.geometry_rigs[geo].ntargets == 0) return rig_fail("model_geometry_targets_get: bad arguments or a geometry without morph targets");
    const LoadedModel::GeometryRig& g = m->m.geometry_rigs[geo];
    if (deltas3) memcpy(deltas3, g.deltas.data(), g.deltas.size() * 4);
    if (default_weights) memcpy(default_weights, g.default_weights.data(), g.default_weights.size() * 4);
    return FRT_OK;
}
int frt_model_nodes_get(const frt_model* m, int32_t* parents, float* rest_trs, uint8_t* has_matrix, float* matrices, uint32_t* document_index) {
    if (!m) return rig_fail("model_nodes_get: null");
    for (size_t i = 0; i < m->m.nodes.size(); ++i) {
        const LoadedModel::Node& n = m->m.nodes[i];
        if (parents) parents[i] = n.parent;
        if (rest_trs) memcpy(rest_trs + 10 * i, n.trs, 40);
        if (has_matrix) has_matrix[i] = n.has_matrix ? 1 : 0;
        if (matrices) memcpy(matrices + 16 * i, n.matrix, 64);
        if (document_index) document_index[i] = n.doc_index;
    }
    return FRT_OK;
}
int frt_model_skin_get(const frt_model* m, uint32_t skin, uint32_t* njoints, uint32_t* joint_nodes, float* inverse_bind) {
    if (!m || skin >= m->m.skins.size()) return rig_fail("model_skin_get: bad arguments");
    const LoadedModel::Skin& s = m->m.skins[skin];
    if (njoints) *njoints = (uint32_t)s.joints.size();
    if (joint_nodes) memcpy(joint_nodes, s.joints.data(), s.joints.size() * 4);
    if (inverse_bind) memcpy(inverse_bind, s.inverse_bind.data(), s.inverse_bind.size() * 4);
    return FRT_OK;
}
int frt_model_animation_info(const frt_model* m, uint32_t anim, const char** name_out, uint32_t* nchannels) {
    if (!m || anim >= m->m.animations.size()) return rig_fail("model_animation_info: bad arguments");
    if (name_out) *name_out = m->m.animations[anim].name.c_str();
    if (nchannels) *nchannels = (uint32_t)m->m.animations[anim].channels.size();
    return FRT_OK;
}
int frt_model_channel_info(const frt_model* m, uint32_t anim, uint32_t channel, uint32_t out[5]) {
    if (!m || !out || anim >= m->m.animations.size() || channel >= m->m.animations[anim].channels.size()) return rig_fail("model_channel_info: bad arguments");
    const LoadedModel::Channel& c = m->m.animations[anim].channels[channel];
    out[0] = c.node; out[1] = c.path; out[2] = c.interpolation; out[3] = (uint32_t)c.times.size(); out[4] = (uint32_t)c.values.size();
    return FRT_OK;
}
int frt_model_channel_get(const frt_model* m, uint32_t anim, uint32_t channel, float* times, float* values) {
    if (!m || anim >= m->m.animations.size() || channel >= m->m.animations[anim].channels.size()) return rig_fail("model_channel_get: bad arguments");
    const LoadedModel::Channel& c = m->m.animations[anim].channels[channel];
    if (times) memcpy(times, c.times.data(), c.times.size() * 4);
    if (values) memcpy(values, c.values.data(), c.values.size() * 4);
    return FRT_OK;
}
// The rig of skin `skin_index` (or, with -1, a morph-only rig) of a loaded document: every node, the skin's joints and inverse binds, the targets and
// default weights of the first geometry under that skin (with -1: of the first geometry) that has targets, and one clip per animation in document
// order; a weights channel is taken when its node carries a mesh with that many targets.
// (`nodes_only`, frt_rig_from_model_nodes: no joints, no targets, the weights channels left out, created with FRT_RIG_NODES_ONLY)
static frt_rig* rig_from_model(const frt_model* m, int32_t skin_index, bool nodes_only) {
    if (!m) { rig_fail("rig_from_model: null"); return nullptr; }
    const LoadedModel& L = m->m;
    if (skin_index < -1 || (skin_index >= 0 && (size_t)skin_index >= L.skins.size())) { rig_fail("rig_from_model: skin " + std::to_string(skin_index) + " out of range (" + std::to_string(L.skins.size()) + " skins)"); return nullptr; }
    if (L.nodes.empty()) { rig_fail("rig_from_model: the model has no nodes"); return nullptr; }
    const LoadedModel::GeometryRig* morph = nullptr;
    if (!nodes_only) for (const LoadedModel::GeometryRig& g : L.geometry_rigs) if (g.ntargets && (skin_index < 0 || g.skin == skin_index)) { morph = &g; break; }
    const size_t N = L.nodes.size();
    std::vector<int32_t> parents(N); std::vector<float> trs(10 * N), mats(16 * N); std::vector<uint8_t> has(N);
    frt_model_nodes_get(m, parents.data(), trs.data(), has.data(), mats.data(), nullptr);
    std::vector<std::vector<frt_rig_channel>> channels(L.animations.size());
    std::vector<frt_rig_clip> clips(L.animations.size());
    for (size_t a = 0; a < L.animations.size(); ++a) {
        for (const LoadedModel::Channel& c : L.animations[a].channels) {
            if (c.path == (uint32_t)kRigPathWeights) {
                const int mesh = L.nodes[c.node].mesh;
                if (!morph || mesh != morph->mesh || c.values.size() != c.times.size() * morph->ntargets * (c.interpolation == (uint32_t)kRigCubic ? 3u : 1u)) continue;
            }
            channels[a].push_back(frt_rig_channel{c.node, c.path, c.interpolation, (uint32_t)c.times.size(), c.times.data(), c.values.data()});
        }
        clips[a] = frt_rig_clip{L.animations[a].name.c_str(), (uint32_t)channels[a].size(), channels[a].data()};
    }
    frt_rig_desc d;
    memset(&d, 0, sizeof(d));
    d.nnodes = (uint32_t)N; d.parents = parents.data(); d.rest_trs = trs.data(); d.has_matrix = has.data(); d.matrices = mats.data();
    if (skin_index >= 0) { const LoadedModel::Skin& s = L.skins[(size_t)skin_index]; d.njoints = (uint32_t)s.joints.size(); d.joint_nodes = s.joints.data(); d.inverse_bind = s.inverse_bind.data(); }
    if (morph) { d.ntargets = morph->ntargets; d.default_weights = morph->default_weights.data(); }
    d.nclips = (uint32_t)clips.size(); d.clips = clips.data();
    return frt_rig_create_ex(&d, nodes_only ? FRT_RIG_NODES_ONLY : 0u);
}
frt_rig* frt_rig_from_model(const frt_model* m, int32_t skin_index) { return rig_from_model(m, skin_index, false); }
frt_rig* frt_rig_from_model_nodes(const frt_model* m) { return rig_from_model(m, -1, true); }

int frt_model_geometry_nodes(const frt_model* m, uint32_t geo, uint32_t cap, uint32_t* nodes_out, uint32_t* count_out) {
    if (!m || !count_out || geo >= m->m.geometries.size() || (cap && !nodes_out)) return rig_fail("model_geometry_nodes: bad arguments");
    uint32_t n = 0;
    if (geo < m->m.geometry_rigs.size() && m->m.geometry_rigs[geo].mesh >= 0)      // (an OBJ model has no nodes)
        for (size_t i = 0; i < m->m.nodes.size(); ++i)
            if (m->m.nodes[i].mesh == m->m.geometry_rigs[geo].mesh) { if (n < cap) nodes_out[n] = (uint32_t)i; ++n; }
    *count_out = n;
    return FRT_OK;
}

void frt_acosf(uint32_t n, const float* x, float* out) { for (uint32_t i = 0; i < n; ++i) out[i] = acosf_(x[i]); }

int frt_rig_counts(const frt_rig* rig, uint32_t counts[4]) {
    if (!rig || !counts) return rig_fail("rig_counts: null");
    const RigHeader h = rig->view().h();
    counts[0] = h.nnodes; counts[1] = h.njoints; counts[2] = h.ntargets; counts[3] = h.nclips;
    return FRT_OK;
}

int frt_rig_clip_info(const frt_rig* rig, uint32_t clip, const char** name_out, float* duration_out) {
    if (!rig) return rig_fail("rig_clip_info: null");
    if (clip >= rig->clip_names.size()) return rig_fail("rig_clip_info: clip " + std::to_string(clip) + " out of range (" + std::to_string(rig->clip_names.size()) + " clips)");
    if (name_out) *name_out = rig->clip_names[clip].c_str();
    if (duration_out) *duration_out = rig->clip_durations[clip];
    return FRT_OK;
}

int frt_rig_evaluate(const frt_rig* rig, uint32_t clip, float time, float* joint_mats_out, float* morph_weights_out) {
    if (!rig) return rig_fail("rig_evaluate: null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    if (clip >= h.nclips) return rig_fail("rig_evaluate: clip " + std::to_string(clip) + " out of range (" + std::to_string(h.nclips) + " clips)");
    if (!std::isfinite(time)) return rig_fail("rig_evaluate: time is not finite");
    if ((h.njoints && !joint_mats_out) || (h.ntargets && !morph_weights_out)) return rig_fail("rig_evaluate: null output");
    if (h.njoints) {
        std::vector<m4> global(h.nnodes);
        for (uint32_t n = 0; n < h.nnodes; ++n) {      // parents first
            const m4 local = rig_local_matrix(v, clip, n, time);
            const uint32_t p = v.w[h.parent + n];
            global[n] = p == kRigNone ? local : mul(global[p], local);
        }
        for (uint32_t j = 0; j < h.njoints; ++j) {
            const m4 m = mul(global[v.w[h.joint_node + j]], load_m4(v.f(h.inv_bind) + (size_t)16 * j));
            memcpy(joint_mats_out + (size_t)16 * j, &m, 64);
        }
    }
    for (uint32_t c = 0; c < h.ntargets; ++c) morph_weights_out[c] = rig_morph_weight(v, clip, c, time);
    return FRT_OK;
}

// The specification of rig_nodes_kernel (frt_animation.hip): the globals of frt_rig_evaluate, then rig_node_matrix per queried node.
int frt_rig_evaluate_nodes(const frt_rig* rig, uint32_t clip, float time, uint32_t n, const uint32_t* nodes, const float* root, const float* offsets, float* mats_out) {
    if (!rig) return rig_fail("rig_evaluate_nodes: null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    if (clip >= h.nclips) return rig_fail("rig_evaluate_nodes: clip " + std::to_string(clip) + " out of range (" + std::to_string(h.nclips) + " clips)");
    if (!std::isfinite(time)) return rig_fail("rig_evaluate_nodes: time is not finite");
    if (n == 0 || !nodes || !mats_out) return rig_fail("rig_evaluate_nodes: n is 0, or null nodes or output");
    for (uint32_t k = 0; k < n; ++k)
        if (nodes[k] >= h.nnodes) return rig_fail("rig_evaluate_nodes: node " + std::to_string(nodes[k]) + " is not a node (" + std::to_string(h.nnodes) + " nodes)");
    if (root && !all_finite(root, 16)) return rig_fail("rig_evaluate_nodes: a root entry is not finite");
    if (offsets && !all_finite(offsets, (size_t)16 * n)) return rig_fail("rig_evaluate_nodes: an offsets entry is not finite");
    std::vector<m4> global(h.nnodes);
    for (uint32_t i = 0; i < h.nnodes; ++i) {      // parents first
        const m4 local = rig_local_matrix(v, clip, i, time);
        const uint32_t p = v.w[h.parent + i];
        global[i] = p == kRigNone ? local : mul(global[p], local);
    }
    for (uint32_t k = 0; k < n; ++k) {
        const m4 M = rig_node_matrix(global[rig->place[nodes[k]]], root, offsets ? offsets + (size_t)16 * k : nullptr);
        memcpy(mats_out + (size_t)16 * k, &M, 64);
    }
    return FRT_OK;
}

// "Blending clips": the specification of the kernels run with a list of samples. The globals of a checked blend, node by node, parents first.
static std::vector<m4> blend_globals(const RigView& v, const RigHeader& h, uint32_t n, const frt_clip_sample* samples) {
    std::vector<m4> global(h.nnodes);
    for (uint32_t i = 0; i < h.nnodes; ++i) {
        const m4 local = rig_local_matrix_blend(v, n, samples, i);
        const uint32_t p = v.w[h.parent + i];
        global[i] = p == kRigNone ? local : mul(global[p], local);
    }
    return global;
}

int frt_rig_evaluate_blend(const frt_rig* rig, uint32_t n, const frt_clip_sample* samples, float* joint_mats_out, float* morph_weights_out) {
    if (!rig) return rig_fail("rig_evaluate_blend: null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    const std::string bad = check_blend_samples(n, samples, h.nclips);
    if (!bad.empty()) return rig_fail("rig_evaluate_blend: " + bad);
    if ((h.njoints && !joint_mats_out) || (h.ntargets && !morph_weights_out)) return rig_fail("rig_evaluate_blend: null output");
    if (h.njoints) {
        const std::vector<m4> global = blend_globals(v, h, n, samples);
        for (uint32_t j = 0; j < h.njoints; ++j) {
            const m4 m = mul(global[v.w[h.joint_node + j]], load_m4(v.f(h.inv_bind) + (size_t)16 * j));
            memcpy(joint_mats_out + (size_t)16 * j, &m, 64);
        }
    }
    for (uint32_t c = 0; c < h.ntargets; ++c) morph_weights_out[c] = rig_morph_weight_blend(v, n, samples, c);
    return FRT_OK;
}

int frt_rig_evaluate_nodes_blend(const frt_rig* rig, uint32_t n, const frt_clip_sample* samples, uint32_t nnodes, const uint32_t* nodes, const float* root, const float* offsets, float* mats_out) {
    if (!rig) return rig_fail("rig_evaluate_nodes_blend: null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    const std::string bad = check_blend_samples(n, samples, h.nclips);
    if (!bad.empty()) return rig_fail("rig_evaluate_nodes_blend: " + bad);
    if (nnodes == 0 || !nodes || !mats_out) return rig_fail("rig_evaluate_nodes_blend: nnodes is 0, or null nodes or output");
    for (uint32_t k = 0; k < nnodes; ++k)
        if (nodes[k] >= h.nnodes) return rig_fail("rig_evaluate_nodes_blend: node " + std::to_string(nodes[k]) + " is not a node (" + std::to_string(h.nnodes) + " nodes)");
    if (root && !all_finite(root, 16)) return rig_fail("rig_evaluate_nodes_blend: a root entry is not finite");
    if (offsets && !all_finite(offsets, (size_t)16 * nnodes)) return rig_fail("rig_evaluate_nodes_blend: an offsets entry is not finite");
    const std::vector<m4> global = blend_globals(v, h, n, samples);
    for (uint32_t k = 0; k < nnodes; ++k) {
        const m4 M = rig_node_matrix(global[rig->place[nodes[k]]], root, offsets ? offsets + (size_t)16 * k : nullptr);
        memcpy(mats_out + (size_t)16 * k, &M, 64);
    }
    return FRT_OK;
}

} // extern "C"

// "Layering clips": the specification of the kernels run with a list of layers. What both calls check of the list and the masks; the masks in the
// block's node order (`stored`; the caller gives them in its own); the globals of a checked list, node by node, parents first.
static std::string check_layers_call(const frt_rig* rig, const RigHeader& h, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, std::vector<float>& stored) {
    if (nmasks > FRT_MAX_RIG_MASKS) return std::to_string(nmasks) + " masks, more than FRT_MAX_RIG_MASKS";
    std::string bad = check_clip_layers(n, layers, h.nclips, nmasks);
    if (bad.empty()) bad = check_rig_masks(nmasks, masks, h.nnodes);
    if (!bad.empty()) return bad;
    stored.resize((size_t)nmasks * h.nnodes);
    for (uint32_t m = 0; m < nmasks; ++m)
        for (uint32_t i = 0; i < h.nnodes; ++i) stored[(size_t)m * h.nnodes + rig->place[i]] = masks[(size_t)m * h.nnodes + i];
    return "";
}
// "Inverse kinematics": what both _ik calls check of their goals and targets (`gs`: the goals with stored indices; `tree`: filled when there are any),
// and the goals applied to the globals in list order, each from the globals the earlier ones left: the text of rig_apply_goals (frt_animation.hip).
static std::string check_goals_call(const frt_rig* rig, uint32_t ngoals, const frt_rig_goal* goals, const frt_rig_goal_target* targets, std::vector<frt_rig_goal>& gs, RigTree& tree) {
    if (ngoals > FRT_MAX_RIG_GOALS) return std::to_string(ngoals) + " goals, more than FRT_MAX_RIG_GOALS";
    if (ngoals == 0) return "";
    tree = rig_tree(rig->view());
    const std::string bad = check_rig_goals(ngoals, goals, rig->place, tree.enter.data(), tree.exit.data(), gs);
    return bad.empty() ? check_rig_goal_targets(ngoals, targets, ngoals, gs.data()) : bad;
}
// "Chain IK": one chain goal in its stored form (mid: the sweeps; reserved: K, the bones of the path), over arrays where rig_apply_chain
// (frt_animation.hip) holds the chain in the lanes of a wave. `parent`: the block's parents, stored order.
static void apply_chain_goal(std::vector<m4>& global, const frt_rig_goal& g, const frt_rig_goal_target& t, const RigTree& tree, const uint32_t* parent) {
    if (!ik_target_ok(t)) return;
    const uint32_t K = g.reserved, S = g.mid;
    std::vector<uint32_t> c(K + 1u);
    c[K] = g.tip;
    for (uint32_t j = K; j-- > 0u;) c[j] = parent[c[j + 1u]];      // (check_rig_goals has counted the path: c[0] is the root)
    std::vector<f3> P(K + 1u);
    std::vector<m4> D(K + 1u, ik_identity());
    for (uint32_t j = 0; j <= K; ++j) P[j] = xyz(global[c[j]].c[3]);
    const f3 Te = ik_chain_target(P[K], t);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t k = K; k-- > 0u;) {
            m4 R;
            if (!ik_chain_step(P[k], P[K], Te, R)) continue;
            for (uint32_t j = k + 1u; j <= K; ++j) P[j] = ik_point(R, P[j]);
            for (uint32_t j = k; j <= K; ++j) D[j] = mul(R, D[j]);
        }
    const uint32_t* enter = tree.enter.data(); const uint32_t* exit = tree.exit.data();
    for (uint32_t n = 0; n < (uint32_t)global.size(); ++n) {
        if (!ik_in_subtree(enter, exit, c[0], n)) continue;
        uint32_t j = 0;      // the deepest chain node whose subtree holds n; the tip's own subtree moves with the last bone
        for (uint32_t i = 1u; i <= K; ++i) if (ik_in_subtree(enter, exit, c[i], n)) j = i;
        global[n] = mul(D[j < K ? j : K - 1u], global[n]);
    }
}
static void apply_goals(std::vector<m4>& global, const std::vector<frt_rig_goal>& gs, const frt_rig_goal_target* targets, const RigTree& tree, const uint32_t* parent) {
    for (size_t i = 0; i < gs.size(); ++i) {
        if (gs[i].kind == FRT_GOAL_CHAIN) { apply_chain_goal(global, gs[i], targets[i], tree, parent); continue; }
        const IkDelta d = ik_goal_delta(gs[i], targets[i], global[gs[i].root], global[gs[i].mid], global[gs[i].tip]);
        if (!d.on) continue;
        for (uint32_t n = 0; n < (uint32_t)global.size(); ++n) {
            m4 G = global[n];
            if (ik_move_node(d, tree.enter.data(), tree.exit.data(), n, G)) global[n] = G;
        }
    }
}
static std::vector<m4> layers_globals(const RigView& v, const RigHeader& h, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* stored) {
    std::vector<m4> global(h.nnodes);
    for (uint32_t i = 0; i < h.nnodes; ++i) {
        const m4 local = rig_local_matrix_layers(v, n, layers, nmasks, stored, i);
        const uint32_t p = v.w[h.parent + i];
        global[i] = p == kRigNone ? local : mul(global[p], local);
    }
    return global;
}
static int evaluate_layers(const char* call, const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals,
                           const frt_rig_goal* goals, const frt_rig_goal_target* targets, float* joint_mats_out, float* morph_weights_out) {
    const std::string name = call;
    if (!rig) return rig_fail(name + ": null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    std::vector<float> stored;
    std::vector<frt_rig_goal> gs;
    RigTree tree;
    std::string bad = check_layers_call(rig, h, n, layers, nmasks, masks, stored);
    if (bad.empty()) bad = check_goals_call(rig, ngoals, goals, targets, gs, tree);
    if (!bad.empty()) return rig_fail(name + ": " + bad);
    if ((h.njoints && !joint_mats_out) || (h.ntargets && !morph_weights_out)) return rig_fail(name + ": null output");
    if (h.njoints) {
        std::vector<m4> global = layers_globals(v, h, n, layers, nmasks, stored.data());
        apply_goals(global, gs, targets, tree, v.w + h.parent);
        for (uint32_t j = 0; j < h.njoints; ++j) {
            const m4 m = mul(global[v.w[h.joint_node + j]], load_m4(v.f(h.inv_bind) + (size_t)16 * j));
            memcpy(joint_mats_out + (size_t)16 * j, &m, 64);
        }
    }
    for (uint32_t c = 0; c < h.ntargets; ++c) morph_weights_out[c] = rig_morph_weight_layers(v, n, layers, c);
    return FRT_OK;
}
static int evaluate_nodes_layers(const char* call, const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals,
                                 const frt_rig_goal* goals, const frt_rig_goal_target* targets, uint32_t nnodes, const uint32_t* nodes, const float* root, const float* offsets,
                                 float* mats_out) {
    const std::string name = call;
    if (!rig) return rig_fail(name + ": null");
    const RigView v = rig->view();
    const RigHeader h = v.h();
    std::vector<float> stored;
    std::vector<frt_rig_goal> gs;
    RigTree tree;
    std::string bad = check_layers_call(rig, h, n, layers, nmasks, masks, stored);
    if (bad.empty()) bad = check_goals_call(rig, ngoals, goals, targets, gs, tree);
    if (!bad.empty()) return rig_fail(name + ": " + bad);
    if (nnodes == 0 || !nodes || !mats_out) return rig_fail(name + ": nnodes is 0, or null nodes or output");
    for (uint32_t k = 0; k < nnodes; ++k)
        if (nodes[k] >= h.nnodes) return rig_fail(name + ": node " + std::to_string(nodes[k]) + " is not a node (" + std::to_string(h.nnodes) + " nodes)");
    if (root && !all_finite(root, 16)) return rig_fail(name + ": a root entry is not finite");
    if (offsets && !all_finite(offsets, (size_t)16 * nnodes)) return rig_fail(name + ": an offsets entry is not finite");
    std::vector<m4> global = layers_globals(v, h, n, layers, nmasks, stored.data());
    apply_goals(global, gs, targets, tree, v.w + h.parent);
    for (uint32_t k = 0; k < nnodes; ++k) {
        const m4 M = rig_node_matrix(global[rig->place[nodes[k]]], root, offsets ? offsets + (size_t)16 * k : nullptr);
        memcpy(mats_out + (size_t)16 * k, &M, 64);
    }
    return FRT_OK;
}

extern "C" {

int frt_rig_evaluate_layers(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, float* joint_mats_out, float* morph_weights_out) {
    return evaluate_layers("rig_evaluate_layers", rig, n, layers, nmasks, masks, 0u, nullptr, nullptr, joint_mats_out, morph_weights_out);
}
int frt_rig_evaluate_nodes_layers(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t nnodes, const uint32_t* nodes, const float* root, const float* offsets, float* mats_out) {
    return evaluate_nodes_layers("rig_evaluate_nodes_layers", rig, n, layers, nmasks, masks, 0u, nullptr, nullptr, nnodes, nodes, root, offsets, mats_out);
}
int frt_rig_evaluate_layers_ik(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals, const frt_rig_goal* goals,
                               const frt_rig_goal_target* targets, float* joint_mats_out, float* morph_weights_out) {
    return evaluate_layers("rig_evaluate_layers_ik", rig, n, layers, nmasks, masks, ngoals, goals, targets, joint_mats_out, morph_weights_out);
}
int frt_rig_evaluate_nodes_layers_ik(const frt_rig* rig, uint32_t n, const frt_clip_layer* layers, uint32_t nmasks, const float* masks, uint32_t ngoals, const frt_rig_goal* goals,
                                     const frt_rig_goal_target* targets, uint32_t nnodes, const uint32_t* nodes, const float* root, const float* offsets, float* mats_out) {
    return evaluate_nodes_layers("rig_evaluate_nodes_layers_ik", rig, n, layers, nmasks, masks, ngoals, goals, targets, nnodes, nodes, root, offsets, mats_out);
}

} // extern "C"
