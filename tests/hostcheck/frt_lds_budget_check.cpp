// TEST INFRASTRUCTURE ONLY — not linked into libfrt.so.
// The launch plan of the quad-walk frame kernels' LDS (csrc/frt_kernels.hpp: traced_lds_budget, walk_lds_plan, gbuffer_lds_budget) as the host code
// of the library computes it, for tests/test_lds_budget.py. The walks over a copy of the tree's top are tests/hostcheck/frt_top_cache_check.cpp,
// built into the same checker.
#include "../../fast-raytracing-wgpu_amd/csrc/frt_kernels.hpp"

using namespace frt;

extern "C" {
// out[0 .. 3]: the budget the plan accepted for a traced workgroup that asked for `want` bytes, then the plan under it: stack rows, nodes, bytes.
void lb_traced_plan(uint32_t wg_rows, uint32_t num_nodes4, uint32_t want, uint32_t* out) {
    out[0] = traced_lds_budget(wg_rows, want);
    const WalkLdsPlan p = walk_lds_plan(wg_rows, num_nodes4, out[0]);
    out[1] = p.stack_rows; out[2] = p.top_nodes; out[3] = p.bytes;
}
// out[0 .. 3]: the G-buffer kernel's budget and its plan.
void lb_gbuffer_plan(uint32_t wg_rows, uint32_t num_nodes4, uint32_t* out) {
    out[0] = gbuffer_lds_budget(wg_rows);
    const WalkLdsPlan p = walk_lds_plan(wg_rows, num_nodes4, out[0]);
    out[1] = p.stack_rows; out[2] = p.top_nodes; out[3] = p.bytes;
}
// the constants of the plan: {kLdsTopNodes, shared bytes, granule, default budget, full budget, LDS per CU, default of traced_lds_budget(wg_rows)}
void lb_constants(uint32_t wg_rows, uint32_t* out) {
    out[0] = (uint32_t)kLdsTopNodes; out[1] = kLdsSharedWords * 4u; out[2] = kLdsGranule; out[3] = kLdsSharedBudget; out[4] = kLdsTracedBudget;
    out[5] = kLdsPerCu; out[6] = traced_lds_budget(wg_rows);
}
}
