// TEST TOOL — not loaded by the product. The shading functions of csrc/frt_shade.hpp / frt_path.hpp, one call per case, compiled for gfx950 under the
// product's device flags (built by __graft_entry__.build(); driven by tests/test_wgsl_f64_shade_gpu.py):
//     shade_probe OP in.bin out.bin
// reads the input records of operation OP (tests/hostcheck/frt_shade_probe.hpp: the record layouts and the one probe body), runs one thread per case
// in 256-thread blocks in a single launch, and writes the output records. For nee0 / nee1 the file starts with the table of 100 lights.
// Any failure — usage, file, record count, a HIP status — prints to stderr and exits non-zero.
#include "../tests/hostcheck/frt_shade_probe.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace frt;
using namespace frt::probe;

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) { fprintf(stderr, "shade_probe: %s: %s\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)

__global__ void __launch_bounds__(256) probe_kernel(int op, const LightView* lights, const void* in, void* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    shade_probe_case(op, lights, in, out, i);
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: shade_probe OP in.bin out.bin\n"); return 2; }
    int op = -1;
    for (int k = 0; k < OP_COUNT; ++k) if (!strcmp(argv[1], op_name(k))) op = k;
    if (op < 0) { fprintf(stderr, "shade_probe: unknown operation %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "shade_probe: cannot open %s\n", argv[2]); return 2; }
    std::vector<uint8_t> bytes;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + got);
    fclose(f);
    const bool nee = op == OP_NEE0 || op == OP_NEE1;
    const size_t table = nee ? (size_t)kProbeLights * sizeof(LightView) : 0u;
    const size_t isz = in_size(op), osz = out_size(op);
    if (bytes.size() < table || (bytes.size() - table) % isz != 0 || bytes.size() == table || (bytes.size() - table) / isz > 0x7FFFFFFFu / 256u) {
        fprintf(stderr, "shade_probe: %s holds %zu bytes: not a whole, non-empty number of %zu-byte records\n", argv[2], bytes.size(), isz);
        return 2;
    }
    const uint32_t n = (uint32_t)((bytes.size() - table) / isz);
    if (!nee_records_ok(op, bytes.data() + table, n)) { fprintf(stderr, "shade_probe: a record's num_lights exceeds the table\n"); return 2; }
    uint8_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void**)&d_in, bytes.size()));
    CHECK(hipMalloc((void**)&d_out, (size_t)n * osz));
    CHECK(hipMemcpy(d_in, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, (size_t)n * osz));
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, 0, op, reinterpret_cast<const LightView*>(d_in), (const void*)(d_in + table),
                       (void*)d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint8_t> out((size_t)n * osz);
    CHECK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    FILE* g = fopen(argv[3], "wb");
    if (!g || fwrite(out.data(), 1, out.size(), g) != out.size() || fclose(g) != 0) { fprintf(stderr, "shade_probe: cannot write %s\n", argv[3]); return 2; }
    return 0;
}
