// exact_div_sqrt_check — the device forms of 1 / x, sqrt(x), 1 / sqrt(x) and -1 / x of csrc/frt_math.hpp (rcpf_, sqrtf_, rsqrt_exact, neg_rcpf_) against the
// compiler's correctly rounded expansions, for ALL 2^32 bit patterns of x, both sides evaluated in one kernel under the product's flags
// (built by __graft_entry__.build() with the Makefile's FLAGS; tests/test_exact_div_sqrt_gpu.py). Two NaNs count as equal.
// Prints one JSON line: per form the number of mismatching patterns, the first few of them, and how many patterns took the fast path.
#include "../fast-raytracing-wgpu_amd/csrc/frt_math.hpp"
#include <stdio.h>

namespace {

const int kForms = 4, kFirst = 16;
struct Result { unsigned long long bad[kForms], fast[kForms]; uint32_t n_first[kForms], first[kForms][kFirst]; };

__device__ __forceinline__ bool same(float a, float b) { return frt::f2u(a) == frt::f2u(b) || (a != a && b != b); }

__device__ void report(Result* res, int form, uint32_t bits) {
    if (*(volatile uint32_t*)&res->n_first[form] >= (uint32_t)kFirst) return;
    const uint32_t i = atomicAdd(&res->n_first[form], 1u);
    if (i < (uint32_t)kFirst) res->first[form][i] = bits;
}

// grid (128, 512) x 256 threads: blockIdx.y = sign and exponent, 256 consecutive mantissas per thread
__global__ void check_kernel(Result* res) {
    const uint32_t hi = blockIdx.y << 23, t = blockIdx.x * 256u + threadIdx.x;
    uint32_t bad[kForms] = {0, 0, 0, 0}, fast[kForms] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 256u; ++k) {
        const uint32_t bits = hi | (t * 256u + k);
        const float x = frt::u2f(bits);
        const float want[kForms] = {1.0f / x, __builtin_sqrtf(x), 1.0f / __builtin_sqrtf(x), -1.0f / x};
        const float got[kForms] = {frt::rcpf_(x), frt::sqrtf_(x), frt::rsqrt_exact(x), frt::neg_rcpf_(x)};
        const bool in[kForms] = {frt::rcp_fast_range(x), frt::sqrt_fast_range(x), frt::sqrt_fast_range(x), frt::rcp_fast_range(x)};
        for (int f = 0; f < kForms; ++f) {
            fast[f] += in[f] ? 1u : 0u;
            if (!same(got[f], want[f])) { ++bad[f]; report(res, f, bits); }
        }
    }
    for (int f = 0; f < kForms; ++f) {
        if (bad[f]) atomicAdd(&res->bad[f], (unsigned long long)bad[f]);
        if (fast[f]) atomicAdd(&res->fast[f], (unsigned long long)fast[f]);
    }
}

} // namespace

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    Result* dev = nullptr;
    static Result r;
    CK(hipMalloc(&dev, sizeof(Result)));
    CK(hipMemset(dev, 0, sizeof(Result)));
    check_kernel<<<dim3(128, 512), 256>>>(dev);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(&r, dev, sizeof(Result), hipMemcpyDeviceToHost));
    CK(hipFree(dev));
    const char* names[kForms] = {"rcp", "sqrt", "rsqrt", "neg_rcp"};
    printf("{");
    for (int f = 0; f < kForms; ++f) {
        printf("%s\"%s\": {\"patterns\": 4294967296, \"mismatches\": %llu, \"fast_path\": %llu, \"first\": [", f ? ", " : "", names[f], r.bad[f], r.fast[f]);
        const uint32_t n = r.n_first[f] < (uint32_t)kFirst ? r.n_first[f] : (uint32_t)kFirst;
        for (uint32_t i = 0; i < n; ++i) printf("%s\"0x%08x\"", i ? ", " : "", r.first[f][i]);
        printf("]}");
    }
    printf("}\n");
    return 0;
}
