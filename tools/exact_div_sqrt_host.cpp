// exact_div_sqrt_host — the HOST branch of rcpf_, sqrtf_ and rsqrt_exact (csrc/frt_math.hpp), evaluated on a file of binary32 values:
//   exact_div_sqrt_host <in.f32> <out.f32>      out = rcpf_(x) for every x, then sqrtf_(x) for every x, then rsqrt_exact(x) for every x
// Compiled host-only (hipcc --cuda-host-only, the flags of tests/hostcheck); tests/test_exact_div_sqrt.py compares the output with IEEE
// division and square root computed elsewhere. No GPU is touched.
#include "../fast-raytracing-wgpu_amd/csrc/frt_math.hpp"
#include <stdio.h>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in.f32> <out.f32>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    std::vector<float> x(n), y(3 * n);
    if (fread(x.data(), sizeof(float), n, f) != n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        y[i] = frt::rcpf_(x[i]);
        y[n + i] = frt::sqrtf_(x[i]);
        y[2 * n + i] = frt::rsqrt_exact(x[i]);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    if (fwrite(y.data(), sizeof(float), 3 * n, f) != 3 * n) { fprintf(stderr, "short write\n"); return 1; }
    fclose(f);
    return 0;
}
