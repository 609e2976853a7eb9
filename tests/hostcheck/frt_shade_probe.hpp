// TEST INFRASTRUCTURE ONLY — the one probe body of tests/test_wgsl_f64_shade*.py: one call of one shading function of csrc/frt_shade.hpp /
// frt_path.hpp per case, from a flat input record array into a flat output record array. No tracing, no tree, no frame buffers: the SceneView and the
// FrameView of the PathCtx are zero-initialised and only `lights`, `cam.num_lights` and `max_depth` are set; the shadow ray's answer is an input.
// Included by tools/shade_probe.hip (gfx950, the product's device flags) and by tests/hostcheck/frt_hostcheck.cpp (host build), so that both run
// the same text. The oracle's exports of the same records are oracle/orc_render.cpp: orc_shade_probe.
//
// Record layouts: little-endian, every field a 4-byte word (f32 or u32), no padding. The numpy dtypes are tests/_shade_probe.py: IN / OUT, the one
// definition on the Python side; shade_probe_sizes() below lets the tests compare the sizes of every build with them.
//   light (64 B, = LightView):  position f32[3], type u32, u f32[3], area f32, v f32[3], pad u32, emission f32[4]
//   op            input record                                                                          output record
//   basis         n[3]                                                                                  tangent[3] bitangent[3]
//   fresnel       f0[3] v_dot_h                                                                         f[3]
//   reflectance   cosine ref_idx                                                                        r
//   ndf           n_dot_h roughness                                                                     d
//   g1            n_dot_v roughness                                                                     g
//   vndf          wo[3] roughness u[2]                                                                  wm[3]
//   light         light rng:u32                                                                         pos[3] normal[3] pdf emission[4] rng:u32
//   eval_pdf      n[3] wi[3] wo[3] roughness metallic transmission ior base[3]                          pdf
//   eval_bsdf     (as eval_pdf)                                                                         f[3]
//   unit_vector   rng:u32                                                                               v[3] rng:u32
//   sample_bsdf   wo[3] ffn[3] front:u32 roughness metallic transmission ior base[3] rng:u32            wi[3] pdf weight[3] rng:u32
//   nee0 / nee1   num_lights:u32 pos[3] ffn[3] wo[3] roughness metallic transmission ior base[3]        nee:u32 want:u32 o[3] d[3] tmin tmax direct[3] rng:u32
//                 visible:u32 rng:u32          (the file starts with a table of kProbeLights lights)    (nee: 0 none, 1 zero, 2 trace, 3 visible without a ray)
//   roulette      depth:u32 throughput[3] ffn[3] next_dir[3] pos[3] rng:u32                             survived:u32 throughput[3] origin[3] rng:u32
#pragma once
#include "../../fast-raytracing-wgpu_amd/csrc/frt_path.hpp"

namespace frt {
namespace probe {

enum Op : int { OP_BASIS = 0, OP_FRESNEL, OP_REFLECTANCE, OP_NDF, OP_G1, OP_VNDF, OP_LIGHT, OP_EVAL_PDF, OP_EVAL_BSDF, OP_UNIT_VECTOR, OP_SAMPLE_BSDF,
                OP_NEE0, OP_NEE1, OP_ROULETTE, OP_COUNT };
static constexpr uint32_t kProbeLights = 100u;      // lights in the table in front of the nee records; num_lights of a record is at most this

struct BasisIn { float n[3]; };                                   struct BasisOut { float t[3], b[3]; };
struct FresnelIn { float f0[3], v_dot_h; };                       struct FresnelOut { float f[3]; };
struct ReflectanceIn { float cosine, ref_idx; };                  struct ScalarOut { float v; };
struct NdfIn { float n_dot_h, roughness; };
struct G1In { float n_dot_v, roughness; };
struct VndfIn { float wo[3], roughness, u[2]; };                  struct VndfOut { float wm[3]; };
struct LightIn { LightView light; uint32_t rng; };                struct LightOut { float pos[3], normal[3], pdf, emission[4]; uint32_t rng; };
struct EvalIn { float n[3], wi[3], wo[3], roughness, metallic, transmission, ior, base[3]; };
struct EvalBsdfOut { float f[3]; };
struct UnitIn { uint32_t rng; };                                  struct UnitOut { float v[3]; uint32_t rng; };
struct SampleIn { float wo[3], ffn[3]; uint32_t front; float roughness, metallic, transmission, ior, base[3]; uint32_t rng; };
struct SampleOut { float wi[3], pdf, weight[3]; uint32_t rng; };
struct NeeIn { uint32_t num_lights; float pos[3], ffn[3], wo[3], roughness, metallic, transmission, ior, base[3]; uint32_t visible, rng; };
struct NeeOut { uint32_t nee, want; float o[3], d[3], tmin, tmax, direct[3]; uint32_t rng; };
struct RouletteIn { uint32_t depth; float throughput[3], ffn[3], next_dir[3], pos[3]; uint32_t rng; };
struct RouletteOut { uint32_t survived; float throughput[3], origin[3]; uint32_t rng; };

FRT_HD uint32_t in_size(int op) {
    switch (op) {
    case OP_BASIS: return sizeof(BasisIn); case OP_FRESNEL: return sizeof(FresnelIn); case OP_REFLECTANCE: return sizeof(ReflectanceIn);
    case OP_NDF: return sizeof(NdfIn); case OP_G1: return sizeof(G1In); case OP_VNDF: return sizeof(VndfIn); case OP_LIGHT: return sizeof(LightIn);
    case OP_EVAL_PDF: case OP_EVAL_BSDF: return sizeof(EvalIn); case OP_UNIT_VECTOR: return sizeof(UnitIn); case OP_SAMPLE_BSDF: return sizeof(SampleIn);
    case OP_NEE0: case OP_NEE1: return sizeof(NeeIn); case OP_ROULETTE: return sizeof(RouletteIn);
    }
    return 0u;
}
FRT_HD uint32_t out_size(int op) {
    switch (op) {
    case OP_BASIS: return sizeof(BasisOut); case OP_FRESNEL: return sizeof(FresnelOut);
    case OP_REFLECTANCE: case OP_NDF: case OP_G1: case OP_EVAL_PDF: return sizeof(ScalarOut);
    case OP_VNDF: return sizeof(VndfOut); case OP_LIGHT: return sizeof(LightOut); case OP_EVAL_BSDF: return sizeof(EvalBsdfOut);
    case OP_UNIT_VECTOR: return sizeof(UnitOut); case OP_SAMPLE_BSDF: return sizeof(SampleOut);
    case OP_NEE0: case OP_NEE1: return sizeof(NeeOut); case OP_ROULETTE: return sizeof(RouletteOut);
    }
    return 0u;
}
inline const char* op_name(int op) {
    static const char* names[OP_COUNT] = {"basis", "fresnel", "reflectance", "ndf", "g1", "vndf", "light", "eval_pdf", "eval_bsdf", "unit_vector",
                                          "sample_bsdf", "nee0", "nee1", "roulette"};
    return op >= 0 && op < OP_COUNT ? names[op] : "";
}

FRT_HD f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
FRT_HD void st3(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

template <int VARIANT>
FRT_HD void nee_case(PathCtx& c, const NeeIn& in, NeeOut& o) {
    PathState st;
    path_begin(c, st, 0u, in.rng);
    st.pos = ld3(in.pos); st.ffnormal = ld3(in.ffn); st.wo = ld3(in.wo); st.base_color = ld3(in.base);
    st.m.roughness = in.roughness; st.m.metallic = in.metallic; st.m.transmission = in.transmission; st.m.ior = in.ior;
    AnyReq req; req.want = false; req.o = splat3(0.0f); req.d = splat3(0.0f); req.tmin = 0.0f; req.tmax = 0.0f;
    nee_prepare<VARIANT>(c, st, req);
    o.nee = st.nee; o.want = req.want ? 1u : 0u; st3(o.o, req.o); st3(o.d, req.d); o.tmin = req.tmin; o.tmax = req.tmax;
    o.rng = c.rng;      // before path_post_any, whose sample_bsdf draws on
    // the direct term through path_post_any itself: accum starts at 0 and throughput at 1 (path_begin), so st.accum = 0 + direct * 1 afterwards
    // (a -0 component becomes +0; the oracle's probe adds its term to a zero accumulator alike). What path_post_any does after that is not read.
    path_post_any(c, st, in.visible != 0u);
    st3(o.direct, st.accum);
}

// Case i of `op`. `lights`: the table of kProbeLights lights (nee ops; unused otherwise). The caller has checked i < n and, for the nee ops, that
// every record's num_lights is at most kProbeLights.
FRT_HD void shade_probe_case(int op, const LightView* lights, const void* in_v, void* out_v, uint32_t i) {
    SceneView sv{};
    FrameView fv{};
    fv.max_depth = 8u;
    sv.lights = lights;
    switch (op) {
    case OP_BASIS: {
        const BasisIn& in = static_cast<const BasisIn*>(in_v)[i]; BasisOut& o = static_cast<BasisOut*>(out_v)[i];
        f3 t, b; make_orthonormal_basis(ld3(in.n), t, b); st3(o.t, t); st3(o.b, b);
    } break;
    case OP_FRESNEL: {
        const FresnelIn& in = static_cast<const FresnelIn*>(in_v)[i];
        st3(static_cast<FresnelOut*>(out_v)[i].f, fresnel_schlick(ld3(in.f0), in.v_dot_h));
    } break;
    case OP_REFLECTANCE: {
        const ReflectanceIn& in = static_cast<const ReflectanceIn*>(in_v)[i];
        static_cast<ScalarOut*>(out_v)[i].v = reflectance(in.cosine, in.ref_idx);
    } break;
    case OP_NDF: {
        const NdfIn& in = static_cast<const NdfIn*>(in_v)[i];
        static_cast<ScalarOut*>(out_v)[i].v = ndf_ggx(in.n_dot_h, in.roughness);
    } break;
    case OP_G1: {
        const G1In& in = static_cast<const G1In*>(in_v)[i];
        static_cast<ScalarOut*>(out_v)[i].v = geometry_schlick_ggx(in.n_dot_v, in.roughness);
    } break;
    case OP_VNDF: {
        const VndfIn& in = static_cast<const VndfIn*>(in_v)[i];
        st3(static_cast<VndfOut*>(out_v)[i].wm, sample_ggx_vndf(ld3(in.wo), in.roughness, in.u[0], in.u[1]));
    } break;
    case OP_LIGHT: {
        const LightIn& in = static_cast<const LightIn*>(in_v)[i]; LightOut& o = static_cast<LightOut*>(out_v)[i];
        sv.lights = &in.light;
        PathCtx c(sv, fv, nullptr, 0u); c.rng = in.rng;
        LightSmp s = sample_light(c, 0u);
        st3(o.pos, s.pos); st3(o.normal, s.normal); o.pdf = s.pdf;
        o.emission[0] = s.emission.x; o.emission[1] = s.emission.y; o.emission[2] = s.emission.z; o.emission[3] = s.emission.w; o.rng = c.rng;
    } break;
    case OP_EVAL_PDF: case OP_EVAL_BSDF: {
        const EvalIn& in = static_cast<const EvalIn*>(in_v)[i];
        MatParams m; m.roughness = in.roughness; m.metallic = in.metallic; m.transmission = in.transmission; m.ior = in.ior;
        if (op == OP_EVAL_PDF) static_cast<ScalarOut*>(out_v)[i].v = eval_pdf(ld3(in.n), ld3(in.wi), ld3(in.wo), m, ld3(in.base));
        else st3(static_cast<EvalBsdfOut*>(out_v)[i].f, eval_bsdf(ld3(in.n), ld3(in.wi), ld3(in.wo), m, ld3(in.base)));
    } break;
    case OP_UNIT_VECTOR: {
        UnitOut& o = static_cast<UnitOut*>(out_v)[i];
        PathCtx c(sv, fv, nullptr, 0u); c.rng = static_cast<const UnitIn*>(in_v)[i].rng;
        st3(o.v, random_unit_vector(c)); o.rng = c.rng;
    } break;
    case OP_SAMPLE_BSDF: {
        const SampleIn& in = static_cast<const SampleIn*>(in_v)[i]; SampleOut& o = static_cast<SampleOut*>(out_v)[i];
        MatParams m; m.roughness = in.roughness; m.metallic = in.metallic; m.transmission = in.transmission; m.ior = in.ior;
        PathCtx c(sv, fv, nullptr, 0u); c.rng = in.rng;
        BsdfSmp s = sample_bsdf(c, ld3(in.wo), ld3(in.ffn), in.front != 0u, m, ld3(in.base));
        st3(o.wi, s.wi); o.pdf = s.pdf; st3(o.weight, s.weight); o.rng = c.rng;
    } break;
    case OP_NEE0: case OP_NEE1: {
        const NeeIn& in = static_cast<const NeeIn*>(in_v)[i];
        fv.cam.num_lights = in.num_lights;
        PathCtx c(sv, fv, nullptr, 0u);
        if (op == OP_NEE0) nee_case<0>(c, in, static_cast<NeeOut*>(out_v)[i]); else nee_case<1>(c, in, static_cast<NeeOut*>(out_v)[i]);
    } break;
    case OP_ROULETTE: {
        const RouletteIn& in = static_cast<const RouletteIn*>(in_v)[i]; RouletteOut& o = static_cast<RouletteOut*>(out_v)[i];
        PathCtx c(sv, fv, nullptr, 0u);
        PathState st;
        path_begin(c, st, 0u, in.rng);
        st.depth = in.depth; st.throughput = ld3(in.throughput); st.ffnormal = ld3(in.ffn); st.next_dir = ld3(in.next_dir); st.pos = ld3(in.pos);
        f3 origin = splat3(0.0f);
        o.survived = path_pre_closest(c, st, origin) ? 1u : 0u;
        st3(o.throughput, st.throughput); st3(o.origin, origin); o.rng = c.rng;
    } break;
    default: break;
    }
}

// Host loop over n cases (the host build; the device build launches one thread per case instead). false: a record asks for more lights than the table holds.
inline bool nee_records_ok(int op, const void* in, uint32_t n) {
    if (op != OP_NEE0 && op != OP_NEE1) return true;
    for (uint32_t i = 0; i < n; ++i) if (static_cast<const NeeIn*>(in)[i].num_lights > kProbeLights) return false;
    return true;
}

} // namespace probe
} // namespace frt
