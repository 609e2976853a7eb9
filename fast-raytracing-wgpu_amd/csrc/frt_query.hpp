// frt_query.hpp — ray queries (include/frt.h: frt_scene_trace_*, frt_renderer_trace_*, frt_renderer_pick): caller-supplied rays and
// picked pixels walked through the quad tree by trace4 (frt_trace.hpp), the walk of the frame's kernels. The host form (scene_trace_*) is the
// specification; the kernels of frt_query.hip run the same functions on the device replica and give the same words: which triangle is hit and
// where is decided by the contract triangle test alone, and the record below is assembled from it by copies and one subtraction.
#pragma once
#include "frt_scene.hpp"
#include "frt_kernels.hpp"

namespace frt {

static const uint32_t kQueryMaxRays = 1u << 26;

// A ray the walk is never started for (it is a miss): a non-finite origin or direction component, an all-zero direction, a NaN tmin / tmax.
// Decided on the bits, identically on host and device. (tmin >= tmax needs no rule: no t lies in an empty interval.)
FRT_HD bool query_finite(float x) { return (f2u(x) & 0x7F800000u) != 0x7F800000u; }
FRT_HD bool query_nan(float x) { return (f2u(x) & 0x7FFFFFFFu) > 0x7F800000u; }
FRT_HD bool query_ray_ok(f3 o, f3 d, float tmin, float tmax) {
    const bool finite = query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) && query_finite(d.z);
    const bool zero = ((f2u(d.x) | f2u(d.y) | f2u(d.z)) & 0x7FFFFFFFu) == 0u;
    return finite && !zero && !query_nan(tmin) && !query_nan(tmax);
}

// frt_ray_hit as two 16-byte halves: (t, u, v, tri) (instance, material, primitive, front); a miss is (-1, 0, 0, 0xFFFFFFFF) (0, 0, 0, 0).
FRT_HD void query_hit_record(const SceneView& sc, const HitRec& h, uint4& a, uint4& b) {
    if (h.tri == 0xFFFFFFFFu) {
        a = make_uint4(f2u(-1.0f), 0u, 0u, 0xFFFFFFFFu);
        b = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 in = *reinterpret_cast<const uint4*>(sc.instances + h.inst);      // (mesh, material, first_tri, flip)
    a = make_uint4(f2u(h.t), f2u(h.u), f2u(h.v), h.tri);
    b = make_uint4(h.inst, in.y, h.tri - in.z, h.front ? 1u : 0u);
}

// The host form over a built scene: single-threaded, trace4 compiled for the host over the host copy's quad nodes and triangle slots.
void scene_trace_closest(const SceneBuilder& b, uint32_t n, const frt_ray* rays, frt_ray_hit* out);
void scene_trace_any(const SceneBuilder& b, uint32_t n, const frt_ray* rays, uint8_t* occluded);

// The device form, one thread per ray, asynchronous on `stream`. `rows`: stack rows of a workgroup's LDS (the quad tree's stack need + the shared row),
// `vote`: the voting walk — both as the renderer holds them at the time of the call, i.e. for the tree the replica has now.
// rays: n x 32 B; hits: n x 32 B; occluded: n bytes; xy: n x 8 B. All device memory, the 32-byte records 16-byte aligned.
hipError_t launch_query_closest(const SceneView& sc, bool vote, uint32_t rows, uint32_t n, const void* rays, void* hits, hipStream_t stream);
hipError_t launch_query_any(const SceneView& sc, bool vote, uint32_t rows, uint32_t n, const void* rays, void* occluded, hipStream_t stream);
// Picking: the ray of pixel (xy[2i], xy[2i + 1]) comes from primary_ray (frt_shade.hpp), as the G-buffer stage's; a pixel outside W x H is a miss.
hipError_t launch_query_pick(const SceneView& sc, bool vote, uint32_t rows, const CameraView& cam, uint32_t W, uint32_t H, uint32_t n, const void* xy, void* hits,
                             hipStream_t stream);

} // namespace frt
