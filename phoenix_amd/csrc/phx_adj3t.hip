// phx_adj3t.hip -- translation unit of k3_tail_adj3 (phx_mfma_adj3_tail.inc), the launch that follows the third backward
// kernel: a unit of its own so that phx_adj3.hip's flags, compile time and listing stay what they are.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "phx_solver.hpp"
#include "phx_host.hpp"

using namespace phxh;

#include "phx_mfma_common.inc"
#include "phx_mfma_v3common.inc"
#include "phx_mfma_adj3_tail.inc"

namespace phxh {

// By default the tail kernel runs where a launch has at least four trajectory tiles (more than 48 trajectories: every
// wave of a tail workgroup has a tile); below that (the reference's own batch of 17, 32-trajectory shards) the solve
// keeps its visits and k3_reduce_grads sums, which measured 5 us per step faster there.  PHX_V3_TAIL (diagnostic): 0 =
// never -- k1_solve_adj3 defers nothing, as before the tail kernel --, 1 = wherever the records fit.  A plan whose groups'
// records would not fit the head of a partial (never at H <= 48: a gene block's accumulators alone are 6 144 floats)
// keeps the old path too.
bool adj3_tail_on(const SolveArgs &a)
{
    const char *e = getenv("PHX_V3_TAIL");
    if (e && e[0] == '0') return false;
    const bool forced = e && e[0] == '1';
    return a.grads && a.d.HT == 3 && a.d.TG <= 256 && (forced || a.d.TG * a.d.ntg >= 4) &&
           (long long)tail_record_floats(a.d.Bt, a.d.ntg) <= a.PP;
}

bool launch_adj3_tail(const SolveArgs &a, const phx_grads *g, int overwrite, hipStream_t st)
{
    const D1 &d = a.d;
    hipLaunchKernelGGL((k3_tail_adj3<3>), dim3((unsigned int)(2 * d.nblk)), dim3(256), 0, st, d, a.w, a.net.g,
                       a.grad_y, a.adj_y0, a.PP, g->Ws, g->Wp, g->WaT, g->g, g->bs, g->bp, overwrite, g->Wa);
    return hipGetLastError() == hipSuccess;
}

}  // namespace phxh

extern "C" int phx_debug_adj3_tail_words(size_t *deferred, size_t *served)
{
    // (the header region is the first of every layout: make_regions, phx_plan.hpp)
    if (deferred) *deferred = (size_t)XH_DEFER * 4;
    if (served) *served = (size_t)XH_SERVED * 4;
    const char *e = getenv("PHX_V3_TAIL");
    return (e && e[0] == '0') ? 0 : 1;
}
