// phx_adj3r.hip -- the CLAMP forms of k1_solve_adj3 (phx_mfma_adj3.inc): the backward solve of a batch whose trajectory
// rows each hold a set of up to PHX_CLAMP_MAX genes (phx_odeint_adjoint_backward_clamped_rows).  A translation unit of its
// own, beside phx_adj3.hip and with that unit's flags: the forms of phx_adj3.hip compile as before.  The backend is
// phx_adj3.hip's in plan (without the choice against k1_solve_adj2: no other backward kernel has the mask), layout and
// LDS; a clamped launch never runs the tail kernel (flag bit 8 off), its partials go through k3_reduce_grads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "phx_solver.hpp"
#include "phx_host.hpp"

using namespace phxh;

#include "phx_mfma_common.inc"
#include "phx_mfma_v3common.inc"
#include "phx_mfma_adj3.inc"
#include "phx_plan.hpp"

namespace {

Regions layout_adj3r(const D1 &d, bool grads) { return adj3_backend().layout(d, grads); }
size_t lds_adj3r(const D1 &d) { return adj3_backend().lds(d); }

const void *prepare_adj3r(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    if (!a.clamp) return nullptr;   // the forms without a list are phx_adj3.hip's
    pack_images(a, p, st);
    const char *eh = getenv("PHX_V3_HALF");   // (as prepare_adj3)
    const bool half = p->H <= 16 * (d.HT - 1) + 8 && !(eh && eh[0] == '0');
    const bool split = v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1;
    return split ? (half ? reinterpret_cast<const void *>(k1_solve_adj3<3, true, true, true>)
                         : reinterpret_cast<const void *>(k1_solve_adj3<3, false, true, true>))
                 : (half ? reinterpret_cast<const void *>(k1_solve_adj3<3, true, false, true>)
                         : reinterpret_cast<const void *>(k1_solve_adj3<3, false, false, true>));
}

hipError_t launch_adj3r(const void *fn, const SolveArgs &a, hipStream_t st)
{
    const int flags = a.grads | (a.w.prof_level == 2 ? 2 : 0) | (a.w.prof_level == 3 ? 4 : 0);   // (bit 8 off: no tail kernel)
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved,
                             a.grad_y, a.adj_y0, a.status, a.nfe, a.nsteps, flags, a.PP, a.clamp, a.clamp_width);
}

bool reduce_adj3r(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    const D1 &d = a.d;
    const long long total = (long long)d.nblk * (4 * d.HT * 2 * 64) + d.N + 2 * d.H;
    hipLaunchKernelGGL((k3_reduce_grads<3>), dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, st, a.w.dtheta, npart,
                       a.PP, d.N, d.H, d.nblk, g->Ws, g->Wp, g->WaT, g->g, g->bs, g->bp, overwrite, g->Wa);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

namespace phxh {
const Backend &adj3_rows_backend()
{
    static const Backend b = {3, true, false, true, plan_adj3_any, layout_adj3r, lds_adj3r, plan6_ht, prepare_adj3r,
                              launch_adj3r, reduce_adj3r};
    return b;
}
}  // namespace phxh
