// frt_query.hip — kernels and host form of the ray queries (frt_query.hpp).
// Built with the library's contract flags: the triangle test is trace4's (frt_trace.hpp), the primary ray is the G-buffer stage's (frt_shade.hpp:
// primary_ray), and nothing here adds arithmetic to either beyond `tri - first_tri`.
//
// Launch shape: one thread per ray in the caller's order, blocks of kBlock. Dynamic LDS as the traced kernels lay theirs out — a traversal-stack
// column per thread, `stride` kBlock words (lane-consecutive: conflict-free), and behind the stack rows the shared row that holds the staged top of
// the quad tree (frt_kernels.hpp: stage_top_nodes; one barrier) — but only as many stack rows as the replica's tree needs NOW (rows = stack need + 1,
// read from the renderer at launch), not the frame kernels' fixed 32: the Cornell Box needs 11 KiB of the 32 KiB. A lane without a ray to walk
// (index past n, a degenerate ray, a pixel outside the frame) walks a ray that no box admits instead of leaving: every lane reaches the barrier and
// takes part in the ballots of the staged-top loop and of the voting walk.
#include "frt_query.hpp"
#include "frt_renderer_state.hpp"      // frt::set_error

namespace frt {

static constexpr int kBlock = 256;
extern __shared__ uint32_t s_query[];      // rows x kBlock words

template <bool ANY, bool VOTE>
__device__ __forceinline__ void query_walk(const SceneView& sc, uint32_t rows, bool live, f3 o, f3 d, float tmin, float tmax, HitRec& h) {
    uint32_t* const s_cnt = s_query + (rows - 1u) * (uint32_t)kBlock;
    const uint32_t* const lds_top = stage_top_nodes(sc, s_cnt);
    __syncthreads();
    if (!(live && query_ray_ok(o, d, tmin, tmax))) { o = mk3(0.0f, 0.0f, 0.0f); d = mk3(0.0f, 0.0f, 1.0f); tmin = 1.0f; tmax = 0.0f; }      // empty interval: no box, no triangle
    trace4<ANY, VOTE>(sc, o, d, tmin, tmax, s_query + threadIdx.x, (uint32_t)kBlock, h, lds_top);
}

template <bool ANY, bool VOTE>
__global__ void __launch_bounds__(kBlock) query_rays_kernel(SceneView sc, uint32_t rows, uint32_t n, const float4* __restrict__ rays, uint4* __restrict__ hits,
                                                            uint8_t* __restrict__ occluded) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool have = i < n;
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
    if (have) { q0 = rays[2u * (size_t)i]; q1 = rays[2u * (size_t)i + 1u]; }
    HitRec h;
    query_walk<ANY, VOTE>(sc, rows, have, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), q0.w, q1.w, h);
    if (!have) return;
    if (ANY) { occluded[i] = h.tri != 0xFFFFFFFFu ? (uint8_t)1 : (uint8_t)0; return; }
    uint4 a, b;
    query_hit_record(sc, h, a, b);
    hits[2u * (size_t)i] = a; hits[2u * (size_t)i + 1u] = b;
}

template <bool VOTE>
__global__ void __launch_bounds__(kBlock) query_pick_kernel(SceneView sc, CameraView cam, uint32_t W, uint32_t H, uint32_t rows, uint32_t n,
                                                            const uint2* __restrict__ xy, uint4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool have = i < n;
    uint2 p = make_uint2(0u, 0u);
    if (have) p = xy[i];
    const bool inside = have && p.x < W && p.y < H;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = o;
    if (inside) primary_ray(cam, W, H, p.x, p.y, o, d);
    HitRec h;
    query_walk<false, VOTE>(sc, rows, inside, o, d, kPrimaryTmin, kPrimaryTmax, h);
    if (!have) return;
    uint4 a, b;
    query_hit_record(sc, h, a, b);
    hits[2u * (size_t)i] = a; hits[2u * (size_t)i + 1u] = b;
}

// At least one stack row beside the shared row (a tree of one node needs no stack entry), at most the frame kernels' array.
static uint32_t lds_rows(uint32_t rows) { return rows < 2u ? 2u : (rows > (uint32_t)kStackDepth ? (uint32_t)kStackDepth : rows); }
static dim3 grid_for(uint32_t n) { return dim3((n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock); }

hipError_t launch_query_closest(const SceneView& sc, bool vote, uint32_t rows, uint32_t n, const void* rays, void* hits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    rows = lds_rows(rows);
    const uint32_t lds = rows * (uint32_t)kBlock * 4u;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), lds, stream, sc, rows, n, (const float4*)rays, (uint4*)hits, (uint8_t*)nullptr); };
    if (vote) go(query_rays_kernel<false, true>); else go(query_rays_kernel<false, false>);
    return hipGetLastError();
}
hipError_t launch_query_any(const SceneView& sc, bool vote, uint32_t rows, uint32_t n, const void* rays, void* occluded, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    rows = lds_rows(rows);
    const uint32_t lds = rows * (uint32_t)kBlock * 4u;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), lds, stream, sc, rows, n, (const float4*)rays, (uint4*)nullptr, (uint8_t*)occluded); };
    if (vote) go(query_rays_kernel<true, true>); else go(query_rays_kernel<true, false>);
    return hipGetLastError();
}
hipError_t launch_query_pick(const SceneView& sc, bool vote, uint32_t rows, const CameraView& cam, uint32_t W, uint32_t H, uint32_t n, const void* xy, void* hits,
                             hipStream_t stream) {
    if (n == 0) return hipSuccess;
    rows = lds_rows(rows);
    const uint32_t lds = rows * (uint32_t)kBlock * 4u;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), lds, stream, sc, cam, W, H, rows, n, (const uint2*)xy, (uint4*)hits); };
    if (vote) go(query_pick_kernel<true>); else go(query_pick_kernel<false>);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the host form (the specification)
static SceneView host_view(const SceneBuilder& b) {
    SceneView sv{};
    sv.nodes4 = reinterpret_cast<const float4*>(b.quad_nodes.data());
    sv.num_nodes4 = (uint32_t)b.quad_nodes.size();
    sv.tris = reinterpret_cast<const float4*>(b.tri_slots.data());
    sv.num_tris = (uint32_t)b.tri_slots.size();
    sv.instances = reinterpret_cast<const InstanceView*>(b.instances_dev.data());
    return sv;
}
template <bool ANY>
static void host_walk(const SceneView& sv, const frt_ray& r, HitRec& h) {
    const f3 o = mk3(r.origin[0], r.origin[1], r.origin[2]), d = mk3(r.dir[0], r.dir[1], r.dir[2]);
    h.t = -1.0f; h.u = h.v = 0.0f; h.tri = 0xFFFFFFFFu; h.inst = 0u; h.front = false;
    if (!query_ray_ok(o, d, r.tmin, r.tmax)) return;
    uint32_t stack[kStackDepth];
    trace4<ANY, false>(sv, o, d, r.tmin, r.tmax, stack, 1u, h);
}
void scene_trace_closest(const SceneBuilder& b, uint32_t n, const frt_ray* rays, frt_ray_hit* out) {
    const SceneView sv = host_view(b);
    for (uint32_t i = 0; i < n; ++i) {
        HitRec h;
        host_walk<false>(sv, rays[i], h);
        uint4 lo, hi;
        query_hit_record(sv, h, lo, hi);
        memcpy(&out[i], &lo, 16); memcpy(reinterpret_cast<uint8_t*>(&out[i]) + 16, &hi, 16);
    }
}
void scene_trace_any(const SceneBuilder& b, uint32_t n, const frt_ray* rays, uint8_t* occluded) {
    const SceneView sv = host_view(b);
    for (uint32_t i = 0; i < n; ++i) {
        HitRec h;
        host_walk<true>(sv, rays[i], h);
        occluded[i] = h.tri != 0xFFFFFFFFu ? 1 : 0;
    }
}

} // namespace frt

using namespace frt;
static_assert(sizeof(frt_ray) == 32 && sizeof(frt_ray_hit) == 32, "ABI struct sizes");

extern "C" {

static int scene_query_check(const frt_scene* s, uint32_t n, const void* rays, const void* out, const char* what) {
    if (!s) return set_error(FRT_ERR_INVALID_ARG, std::string(what) + ": null scene");
    if (n > kQueryMaxRays) return set_error(FRT_ERR_INVALID_ARG, std::string(what) + ": more than 2^26 rays in one call");
    if (n == 0) return FRT_OK;
    if (!rays || !out) return set_error(FRT_ERR_INVALID_ARG, std::string(what) + ": null pointer");
    if (!s->b.built) return set_error(FRT_ERR_STATE, std::string(what) + ": the scene is not built");
    return FRT_OK;
}
int frt_scene_trace_closest(const frt_scene* s, uint32_t n, const frt_ray* rays, frt_ray_hit* out) {
    const int rc = scene_query_check(s, n, rays, out, "scene trace_closest");
    if (rc || n == 0) return rc;
    scene_trace_closest(s->b, n, rays, out);
    return FRT_OK;
}
int frt_scene_trace_any(const frt_scene* s, uint32_t n, const frt_ray* rays, uint8_t* occluded_out) {
    const int rc = scene_query_check(s, n, rays, occluded_out, "scene trace_any");
    if (rc || n == 0) return rc;
    scene_trace_any(s->b, n, rays, occluded_out);
    return FRT_OK;
}

} // extern "C"
