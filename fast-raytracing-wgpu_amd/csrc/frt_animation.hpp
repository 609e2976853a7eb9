// frt_animation.hpp — the arithmetic of an animated rig (include/frt.h: frt_rig_evaluate, frt_renderer_animate; DESIGN.md §11, "Animation"): sampling a
// channel at a time, the local matrix of a node, the global matrices down the hierarchy, the joint palette. Every function here is FRT_HD and is the one
// text the host form (frt_animation.cpp) and the kernel (frt_animation.hip) both run under the library's contract flags: f32, no contraction, no
// hand-written fma, rcpf_ / rsqrt_exact / sincosf_ / mul(m4, m4) of frt_math.hpp and acosf_ below.
//
// A rig is ONE block of 32-bit words (RigHeader in front, every table at a word offset from the block's start), so the device copy is the host block,
// byte for byte, and both forms read it through the same accessors. Nodes are stored by depth (level 0: the roots), parents in front of their children.
#pragma once
#include "frt_math.hpp"
#include "../../include/frt.h"      // frt_clip_sample, FRT_MAX_BLEND_SAMPLES

namespace frt {

enum { kRigPathTranslation = 0, kRigPathRotation = 1, kRigPathScale = 2, kRigPathWeights = 3 };      // (frt.h: FRT_RIG_PATH_*)
enum { kRigStep = 0, kRigLinear = 1, kRigCubic = 2 };                                                 // (frt.h: FRT_RIG_*)
static const uint32_t kRigNone = 0xFFFFFFFFu;

// acos in the style of frt_math.hpp's sincosf_ (it lives here and not there because the frame kernels' translation unit includes that header, and its
// text is what the committed counter profile is keyed on): Cephes' asinf polynomial. |x| <= 0.5: pi/2 - asin(x); above: 2 asin(sqrt((1 - |x|) / 2)),
// mirrored for x < 0. |x| > 1 is taken as 1; NaN stays NaN. Built from +, -, * and sqrtf_ only (no libm call), so the host and the device give the same
// bits. Against float64 over [-1, 1]: at most 1.25 ulp (tests/test_animation.py; profiles/animation_f64.md).
FRT_HD float acosf_(float x) {
    const float a = fminn(fabsf_(x), 1.0f);
    const bool big = a > 0.5f;
    const float z = big ? (1.0f - a) * 0.5f : a * a;
    const float s = big ? sqrtf_(z) : a;
    float p = 4.2163199048e-2f;
    p = p * z + 2.4181311049e-2f;
    p = p * z + 4.5470025998e-2f;
    p = p * z + 7.4953002686e-2f;
    p = p * z + 1.6666752422e-1f;
    const float r = s + s * z * p;      // asin(s)
    const float pos = big ? r + r : 1.57079637050628662109375f - r;      // acos(|x|)
    if (x != x) return x;
    return x < 0.0f ? 3.1415927410125732421875f - pos : pos;
}

// Word offsets into the block. parent [N] (kRigNone: a root; else a smaller index), kind [N] (1: a matrix node), rest [16 N] (a matrix node: its matrix,
// column-major; else translation xyz, 0, rotation xyzw, scale xyz, 0, and four unused words), level_begin [nlevels + 1], joint_node [J],
// inv_bind [16 J], def_weights [T], clips [4 nclips] (RigClip), channels [8 nchannels] (RigChannel), then per clip its node table [3 N] (the channel of
// each node's translation, rotation and scale, or kRigNone) and the keys.
struct RigHeader {
    uint32_t words, nnodes, njoints, ntargets, nclips, nlevels, nchannels;
    uint32_t parent, kind, rest, level_begin, joint_node, inv_bind, def_weights, clips, channels;
};
struct RigClip { uint32_t node_table, weights_channel, pad0, pad1; };
struct RigChannel { uint32_t node, path, interp, nkeys, times, values, width, pad; };

struct RigView {      // (the records are copied out of the word block: no struct is read through a cast pointer)
    const uint32_t* w;
    FRT_HD RigHeader h() const { RigHeader r; __builtin_memcpy(&r, w, sizeof(r)); return r; }
    FRT_HD const float* f(uint32_t off) const { return reinterpret_cast<const float*>(w + off); }
    FRT_HD RigClip clip(uint32_t c) const { RigClip r; __builtin_memcpy(&r, w + h().clips + 4u * c, sizeof(r)); return r; }
    FRT_HD RigChannel channel(uint32_t c) const { RigChannel r; __builtin_memcpy(&r, w + h().channels + 8u * c, sizeof(r)); return r; }
};

// Where `t` lies among the K >= 1 strictly increasing key times: `k` the key, `between` false when the result is key k itself (t at or before the first
// key, at or behind the last one, or exactly at key k), else u in (0, 1) and dt = times[k + 1] - times[k] for the interval [k, k + 1].
struct RigKey { uint32_t k; bool between; float u, dt; };
FRT_HD RigKey rig_find_key(const float* times, uint32_t K, float t) {
    RigKey r; r.k = 0u; r.between = false; r.u = 0.0f; r.dt = 0.0f;
    if (t <= times[0]) return r;
    if (t >= times[K - 1u]) { r.k = K - 1u; return r; }
    uint32_t lo = 0u, hi = K - 1u;      // times[lo] <= t < times[hi]
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (times[mid] <= t) lo = mid; else hi = mid; }
    r.k = lo;
    if (t == times[lo]) return r;
    r.between = true;
    r.dt = times[lo + 1u] - times[lo];
    r.u = (t - times[lo]) / r.dt;
    return r;
}
// glTF's cubic Hermite spline over one interval: values v0, v1, out-tangent b0 of the first key and in-tangent a1 of the second, tangents scaled by dt.
FRT_HD float rig_hermite(float v0, float b0, float v1, float a1, float u, float dt) {
    const float u2 = u * u, u3 = u2 * u;
    const float h00 = (2.0f * u3 - 3.0f * u2) + 1.0f, h10 = (u3 - 2.0f * u2) + u, h01 = 3.0f * u2 - 2.0f * u3, h11 = u3 - u2;
    return ((h00 * v0 + (dt * h10) * b0) + h01 * v1) + (dt * h11) * a1;
}
// Component c of a channel of `width` components at the place `key`. The values of a STEP or LINEAR channel are [K][width]; those of a CUBICSPLINE
// channel [K][in-tangent | value | out-tangent][width].
FRT_HD float rig_sample_component(const float* v, uint32_t width, uint32_t interp, RigKey key, uint32_t c) {
    if (interp == (uint32_t)kRigCubic) {
        const float* p = v + (size_t)3u * key.k * width;
        if (!key.between) return p[width + c];
        return rig_hermite(p[width + c], p[2u * width + c], p[4u * width + c], p[3u * width + c], key.u, key.dt);
    }
    const float* p = v + (size_t)key.k * width;
    if (!key.between || interp == (uint32_t)kRigStep) return p[c];
    return mixf(p[c], p[width + c], key.u);
}
FRT_HD float rig_dot4(f4 a, f4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
// Spherical interpolation of two rotations the short way round; nearly parallel ones (d > 0.9995) are mixed component-wise and normalised.
FRT_HD f4 rig_slerp(f4 q0, f4 q1, float u) {
    float d = rig_dot4(q0, q1);
    if (d < 0.0f) { q1 = mk4(-q1.x, -q1.y, -q1.z, -q1.w); d = -d; }
    if (d > 0.9995f) {
        const f4 q = mk4(mixf(q0.x, q1.x, u), mixf(q0.y, q1.y, u), mixf(q0.z, q1.z, u), mixf(q0.w, q1.w, u));
        return q * rsqrt_exact(rig_dot4(q, q));
    }
    const float th = acosf_(d);
    float s, c, s0, s1;
    sincosf_(th, s, c);
    const float inv = rcpf_(s);
    sincosf_((1.0f - u) * th, s0, c);
    sincosf_(u * th, s1, c);
    return q0 * (s0 * inv) + q1 * (s1 * inv);
}
FRT_HD f4 rig_sample_rotation(const float* v, uint32_t interp, RigKey key) {
    if (interp == (uint32_t)kRigLinear && key.between) {
        const float* p = v + (size_t)4u * key.k;
        return rig_slerp(mk4(p[0], p[1], p[2], p[3]), mk4(p[4], p[5], p[6], p[7]), key.u);
    }
    const f4 q = mk4(rig_sample_component(v, 4u, interp, key, 0u), rig_sample_component(v, 4u, interp, key, 1u),
                     rig_sample_component(v, 4u, interp, key, 2u), rig_sample_component(v, 4u, interp, key, 3u));
    if (interp == (uint32_t)kRigCubic && key.between) return q * rsqrt_exact(rig_dot4(q, q));
    return q;
}
// T * R * S: the columns of the rotation matrix (the nine products of the quaternion, each written once) scaled by s, the translation in the last column.
FRT_HD m4 rig_trs_matrix(f3 t, f4 q, f3 s) {
    const float x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const float xx = q.x * x2, xy = q.x * y2, xz = q.x * z2, yy = q.y * y2, yz = q.y * z2, zz = q.z * z2, wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
    m4 m;
    m.c[0] = mk4((1.0f - (yy + zz)) * s.x, (xy + wz) * s.x, (xz - wy) * s.x, 0.0f);
    m.c[1] = mk4((xy - wz) * s.y, (1.0f - (xx + zz)) * s.y, (yz + wx) * s.y, 0.0f);
    m.c[2] = mk4((xz + wy) * s.z, (yz - wx) * s.z, (1.0f - (xx + yy)) * s.z, 0.0f);
    m.c[3] = mk4(t.x, t.y, t.z, 1.0f);
    return m;
}
// Translation, rotation and scale of the non-matrix node n under clip `clip` at time t: every path the clip has a channel for sampled, the others at rest.
struct RigTrs { f3 t; f4 q; f3 s; };
FRT_HD RigTrs rig_local_trs(RigView v, uint32_t clip, uint32_t n, float t) {
    const RigHeader h = v.h();
    const float* rest = v.f(h.rest) + (size_t)16u * n;
    RigTrs r;
    r.t = mk3(rest[0], rest[1], rest[2]); r.s = mk3(rest[8], rest[9], rest[10]);
    r.q = mk4(rest[4], rest[5], rest[6], rest[7]);
    const uint32_t* of = v.w + v.clip(clip).node_table + (size_t)3u * n;
    if (of[0] != kRigNone) {
        const RigChannel ch = v.channel(of[0]);
        const RigKey key = rig_find_key(v.f(ch.times), ch.nkeys, t);
        r.t = mk3(rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 0u), rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 1u),
                  rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 2u));
    }
    if (of[1] != kRigNone) {
        const RigChannel ch = v.channel(of[1]);
        r.q = rig_sample_rotation(v.f(ch.values), ch.interp, rig_find_key(v.f(ch.times), ch.nkeys, t));
    }
    if (of[2] != kRigNone) {
        const RigChannel ch = v.channel(of[2]);
        const RigKey key = rig_find_key(v.f(ch.times), ch.nkeys, t);
        r.s = mk3(rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 0u), rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 1u),
                  rig_sample_component(v.f(ch.values), 3u, ch.interp, key, 2u));
    }
    return r;
}
// The local matrix of node n under clip `clip` at time t: a matrix node's matrix; else T * R * S of rig_local_trs.
FRT_HD m4 rig_local_matrix(RigView v, uint32_t clip, uint32_t n, float t) {
    const RigHeader h = v.h();
    if (v.w[h.kind + n]) return load_m4(v.f(h.rest) + (size_t)16u * n);
    const RigTrs r = rig_local_trs(v, clip, n, t);
    return rig_trs_matrix(r.t, r.q, r.s);
}
// Morph weight c: the clip's weights channel sampled, or the default weight.
FRT_HD float rig_morph_weight(RigView v, uint32_t clip, uint32_t c, float t) {
    const uint32_t wc = v.clip(clip).weights_channel;
    if (wc == kRigNone) return v.f(v.h().def_weights)[c];
    const RigChannel ch = v.channel(wc);
    return rig_sample_component(v.f(ch.values), ch.width, ch.interp, rig_find_key(v.f(ch.times), ch.nkeys, t), c);
}

// Blending clips (include/frt.h: frt_rig_evaluate_blend; DESIGN.md §11, "Blending clips"): the samples s [ns] of (clip, time, weight) in the order
// given, ONE running pose. A sample of weight 0 is skipped entirely; the first sample with a positive weight gives the pose as sampled, without
// arithmetic, and W = w; every later one W = W + w, a = w / W, translation and scale mixed per component, the rotation rig_slerp(R, R_s, a). A list
// without a positive weight is refused by every caller (the result here is then the zero pose).
FRT_HD m4 rig_local_matrix_blend(RigView v, uint32_t ns, const frt_clip_sample* s, uint32_t n) {
    const RigHeader h = v.h();
    if (v.w[h.kind + n]) return load_m4(v.f(h.rest) + (size_t)16u * n);
    RigTrs r;
    r.t = mk3(0.0f, 0.0f, 0.0f); r.s = mk3(0.0f, 0.0f, 0.0f); r.q = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    float W = 0.0f;
    bool first = true;
    for (uint32_t i = 0; i < ns; ++i) {
        const float w = s[i].weight;
        if (!(w > 0.0f)) continue;
        const RigTrs x = rig_local_trs(v, s[i].clip, n, s[i].time);
        if (first) { r = x; W = w; first = false; continue; }
        W = W + w;
        const float a = w / W;
        r.t = mk3(mixf(r.t.x, x.t.x, a), mixf(r.t.y, x.t.y, a), mixf(r.t.z, x.t.z, a));
        r.s = mk3(mixf(r.s.x, x.s.x, a), mixf(r.s.y, x.s.y, a), mixf(r.s.z, x.s.z, a));
        r.q = rig_slerp(r.q, x.q, a);
    }
    return rig_trs_matrix(r.t, r.q, r.s);
}
// Morph weight c of a blend: rig_morph_weight of every sample (a clip's defaults included) under the same running mix.
FRT_HD float rig_morph_weight_blend(RigView v, uint32_t ns, const frt_clip_sample* s, uint32_t c) {
    float r = 0.0f, W = 0.0f;
    bool first = true;
    for (uint32_t i = 0; i < ns; ++i) {
        const float w = s[i].weight;
        if (!(w > 0.0f)) continue;
        const float x = rig_morph_weight(v, s[i].clip, c, s[i].time);
        if (first) { r = x; W = w; first = false; continue; }
        W = W + w;
        r = mixf(r, x, w / W);
    }
    return r;
}

// Layering clips (include/frt.h: frt_rig_evaluate_layers; DESIGN.md §11, "Layering clips"). The product a * b of two rotations, every product and
// sum written once, in this order.
FRT_HD f4 rig_qmul(f4 a, f4 b) {
    return mk4(((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
               ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x,
               ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w,
               ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z);
}
// The layers l [nl] in the order given, ONE running pose (T, R, S) with the accumulated blend weight W. Layer 0 (every caller has checked it: BLEND, no
// mask, a positive weight) gives the pose as sampled, without arithmetic, and W = weight, so every node has a base. A later layer has
// e = weight * m, m = 1 or masks[mask * N + n] (`masks`: [nmasks][N] in the block's node order; a mask index that is not below nmasks, FRT_LAYER_NO_MASK
// among them, reads nothing); !(e > 0) skips it for this node with nothing sampled. BLEND: the blend's rule with e for w. OVERRIDE: a = e, at a >= 1
// the pose becomes the sampled one without arithmetic, else the same mix and slerp by a; W stays. ADDITIVE: with Y the reference clip sampled,
// T = T + e (X.t - Y.t), S likewise, R = R * slerp(identity, conj(Y.q) * X.q, e), not renormalised; W stays.
FRT_HD m4 rig_local_matrix_layers(RigView v, uint32_t nl, const frt_clip_layer* l, uint32_t nmasks, const float* masks, uint32_t n) {
    const RigHeader h = v.h();
    if (v.w[h.kind + n]) return load_m4(v.f(h.rest) + (size_t)16u * n);
    RigTrs r = rig_local_trs(v, l[0].clip, n, l[0].time);
    float W = l[0].weight;
#pragma unroll 1
    for (uint32_t i = 1; i < nl; ++i) {
        const float m = l[i].mask < nmasks ? masks[(size_t)l[i].mask * h.nnodes + n] : 1.0f;
        const float e = l[i].weight * m;
        if (!(e > 0.0f)) continue;
        const RigTrs x = rig_local_trs(v, l[i].clip, n, l[i].time);
        if (l[i].mode == (uint32_t)FRT_LAYER_ADDITIVE) {
            const RigTrs y = rig_local_trs(v, l[i].ref_clip, n, l[i].ref_time);
            r.t = mk3(r.t.x + e * (x.t.x - y.t.x), r.t.y + e * (x.t.y - y.t.y), r.t.z + e * (x.t.z - y.t.z));
            r.s = mk3(r.s.x + e * (x.s.x - y.s.x), r.s.y + e * (x.s.y - y.s.y), r.s.z + e * (x.s.z - y.s.z));
            const f4 d = rig_qmul(mk4(-y.q.x, -y.q.y, -y.q.z, y.q.w), x.q);
            r.q = rig_qmul(r.q, rig_slerp(mk4(0.0f, 0.0f, 0.0f, 1.0f), d, e));
            continue;
        }
        float a = e;
        if (l[i].mode == (uint32_t)FRT_LAYER_BLEND) { W = W + e; a = e / W; }
        else if (a >= 1.0f) { r = x; continue; }
        r.t = mk3(mixf(r.t.x, x.t.x, a), mixf(r.t.y, x.t.y, a), mixf(r.t.z, x.t.z, a));
        r.s = mk3(mixf(r.s.x, x.s.x, a), mixf(r.s.y, x.s.y, a), mixf(r.s.z, x.s.z, a));
        r.q = rig_slerp(r.q, x.q, a);
    }
    return rig_trs_matrix(r.t, r.q, r.s);
}
// Morph weight c of the layers: rig_morph_weight folded the same way with e = weight (masks do not apply to targets). Layer 0 gives the base; a later
// layer with FRT_LAYER_KEEP_MORPH or !(e > 0) is skipped; BLEND is the running mix, OVERRIDE the mix by the weight or the layer's value at >= 1,
// ADDITIVE r + e (x - x_ref).
FRT_HD float rig_morph_weight_layers(RigView v, uint32_t nl, const frt_clip_layer* l, uint32_t c) {
    float r = rig_morph_weight(v, l[0].clip, c, l[0].time), W = l[0].weight;
#pragma unroll 1
    for (uint32_t i = 1; i < nl; ++i) {
        const float e = l[i].weight;
        if ((l[i].flags & FRT_LAYER_KEEP_MORPH) || !(e > 0.0f)) continue;
        const float x = rig_morph_weight(v, l[i].clip, c, l[i].time);
        if (l[i].mode == (uint32_t)FRT_LAYER_ADDITIVE) { r = r + e * (x - rig_morph_weight(v, l[i].ref_clip, c, l[i].ref_time)); continue; }
        float a = e;
        if (l[i].mode == (uint32_t)FRT_LAYER_BLEND) { W = W + e; a = e / W; }
        else if (a >= 1.0f) { r = x; continue; }
        r = mixf(r, x, a);
    }
    return r;
}

// The matrix a bound instance takes from the global G of its node ("Node animation"): mul(mul(root, G), offset), the palette's mul. A null `root` or
// `offset` is no multiplication at all (a product with the identity would turn a -0 into +0).
FRT_HD m4 rig_node_matrix(const m4& G, const float* root, const float* offset) {
    m4 M = G;
    if (root) M = mul(load_m4(root), M);
    if (offset) M = mul(M, load_m4(offset));
    return M;
}

} // namespace frt

#include "frt_ik.hpp"      // "Inverse kinematics": goals on the globals, behind the functions above (rig_slerp, rig_trs_matrix, rig_dot4)

// The host side of a rig (frt_animation.cpp): the block and what frt_rig_clip_info returns. `place`: the caller's node index -> the index in the block
// (frt_rig_create stores the nodes by depth), so the node numbers a caller knows stay valid after creation.
#include <string>
#include <vector>
struct frt_rig {
    std::vector<uint32_t> words;
    std::vector<uint32_t> place;
    std::vector<std::string> clip_names;
    std::vector<float> clip_durations;
    frt::RigView view() const { frt::RigView v; v.w = words.data(); return v; }
};

// frt_renderer_animate_cast ("Animating a cast"), the host part that reads no device: what the call checks about its entries and where each entry's
// outputs lie in the one buffer of the call. A caller describes its bindings by CastBinding (frt_animation.hip fills them from the renderer's list).
struct frt_cast_entry;
namespace frt {
struct CastBinding {
    bool live = false; uint32_t kind = 0, nclips = 0, njoints = 0, ntargets = 0;
    const uint32_t* ids = nullptr; uint32_t n = 0;      // the meshes it poses (kind 0) or the instances it moves (kind 1)
};
// "" or why the call is refused: n == 0 or above FRT_MAX_CAST_ENTRIES, null entries, reserved != 0, flag bits outside `allowed_flags`, an unknown or
// unbound binding, a binding named twice, a clip out of range, a time that is not finite, a mesh (of `nmeshes`) two mesh entries would pose, an
// instance (of `ninstances`) two instance entries would move, an id out of range. Every count is checked before the array it sizes is read.
std::string check_cast_entries(uint32_t n, const frt_cast_entry* entries, uint32_t flags, uint32_t allowed_flags, const CastBinding* bindings, size_t nbindings,
                               size_t nmeshes, size_t ninstances);
// Where entry k's outputs begin: `first[k]` counts instances (an instance entry: its ids and matrices) or palette columns of four floats (a mesh
// entry), `first_weight[k]` morph weights. The buffer is [ids: 4 ninst | matrices: 64 ninst | palettes: 16 cols | weights: 4 nweights], every section
// 16-byte aligned. For entries check_cast_entries has accepted.
struct CastLayout {
    std::vector<uint32_t> first, first_weight;
    uint32_t ninst = 0, cols = 0, nweights = 0, nmesh_entries = 0;
    size_t ids_off = 0, mats_off = 0, pal_off = 0, wt_off = 0, bytes = 0;
};
CastLayout cast_layout(uint32_t n, const frt_cast_entry* entries, const CastBinding* bindings);

// "Blending clips": "" or why a sample list is refused for a rig of `nclips` clips: n == 0 or above FRT_MAX_BLEND_SAMPLES, null samples, reserved != 0,
// a clip out of range, a time or a weight that is not finite, a negative weight, no positive weight. The count is checked before the list is read.
std::string check_blend_samples(uint32_t n, const frt_clip_sample* samples, uint32_t nclips);
// frt_renderer_animate_cast_blend: "" or why the call is refused. The counts, every entry's reserved word and its sample range (inside `nsamples`,
// 1 .. FRT_MAX_BLEND_SAMPLES long) first; then check_cast_entries over `plain`, which is filled here with every entry's binding and its first sample's
// clip and time (what cast_layout takes afterwards); then check_blend_samples of every entry's range against its binding's clips.
std::string check_cast_blend_entries(uint32_t n, const frt_cast_blend_entry* entries, uint32_t nsamples, const frt_clip_sample* samples, uint32_t flags,
                                     uint32_t allowed_flags, const CastBinding* bindings, size_t nbindings, size_t nmeshes, size_t ninstances,
                                     std::vector<frt_cast_entry>& plain);

// "Layering clips": "" or why a layer list is refused for a rig of `nclips` clips seen with `nmasks` masks: n == 0 or above FRT_MAX_LAYERS, null
// layers, an unknown mode or flag bit, a clip out of range, a reference clip out of range on an ADDITIVE layer (any other mode: ref_clip and ref_time
// must be 0), a time, reference time or weight that is not finite, a negative weight, an OVERRIDE weight above 1, a mask that is neither
// FRT_LAYER_NO_MASK nor below nmasks, a layer 0 that is not (BLEND, no mask, weight > 0) or that carries FRT_LAYER_KEEP_MORPH (it is the base of the
// morph weights too). The count is checked before the list is read.
std::string check_clip_layers(uint32_t n, const frt_clip_layer* layers, uint32_t nclips, uint32_t nmasks);
// Masks where they enter (frt_rig_evaluate_layers, frt_renderer_set_rig_masks): "" or nmasks above FRT_MAX_RIG_MASKS, null masks with nmasks > 0, a
// value that is not finite or lies outside [0, 1]. The count is checked before the values are read.
std::string check_rig_masks(uint32_t nmasks, const float* masks, uint32_t nnodes);
// frt_renderer_animate_cast_layers: check_cast_blend_entries for layers. `masks_of` [nbindings]: how many masks each binding carries. `plain` takes
// every entry's binding and its layer 0's clip and time.
std::string check_cast_layers_entries(uint32_t n, const frt_cast_layers_entry* entries, uint32_t nlayers, const frt_clip_layer* layers, uint32_t flags,
                                      uint32_t allowed_flags, const CastBinding* bindings, const uint32_t* masks_of, size_t nbindings, size_t nmeshes,
                                      size_t ninstances, std::vector<frt_cast_entry>& plain);

// "Inverse kinematics": the pre-order numbers of a rig's stored nodes (d lies in subtree(a) iff enter[a] <= enter[d] < exit[a]), kept with the goals.
struct RigTree { std::vector<uint32_t> enter, exit; };
RigTree rig_tree(const RigView& v);
// Goals where they enter (frt_rig_evaluate_layers_ik, frt_renderer_set_rig_goals): "" or ngoals above FRT_MAX_RIG_GOALS, null goals with ngoals > 0,
// an unknown kind, reserved != 0, a node (the caller's number, mapped through `place`) out of range, a mid that is not a strict descendant of root,
// a tip that is not a strict descendant of mid, an AIM axis that is not finite or is zero, AIM mid or tip != 0. The count is checked before the
// array is read. `stored` takes the goals with the block's node indices.
std::string check_rig_goals(uint32_t ngoals, const frt_rig_goal* goals, const std::vector<uint32_t>& place, const uint32_t* enter, const uint32_t* exit, std::vector<frt_rig_goal>& stored);
// Host targets where they enter: "" or a count that is not `bound` (the goals they are for, `goals` [bound]), null targets with a count > 0, a word
// that is not finite, a weight outside [0, 1], a pole flag other than 0 or 1, a pole on an AIM record. The count is checked before the array is read.
std::string check_rig_goal_targets(uint32_t ngoals, const frt_rig_goal_target* targets, uint32_t bound, const frt_rig_goal* goals);
}
