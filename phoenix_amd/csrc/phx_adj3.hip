// phx_adj3.hip -- translation unit of the third backward kernel (k1_solve_adj3, phx_mfma_adj3.inc): launch planning,
// workspace layout and the host entry points the C ABI (phx_engine.hip) calls.
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

size_t lds_bytes_adj3(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + ((ctl3_bytes(d.Bt, d.ntg) + 15) & ~(size_t)15) +
           (v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1 ? v3_comb_bytes(d.NW, 4 * d.HT) : 0);
}

// plan_resident for dopri5 with H <= 48: one wave per SIMD (the augmented sweeps need the 512-register budget)
bool plan_adj3(const Shape &s, D1 *out)
{
    const Switches sw = read_switches(SW_ADJ | SW_V3_NB);
    if (sw.adj == 1 || sw.adj == 2) return false;
    D1 best;
    if (!plan_adj3_any(s, &best)) return false;
    // by shape: the many-member exchange of a narrow hidden layer (the breast-cancer shape) is this kernel's; groups of
    // up to 32 gene tiles stay with the wave-pair kernel (k1_solve_adj2), which is faster there.  PHX_ADJ=v3 forces it.
    if (sw.adj != 3 && best.G <= 32) return false;
    *out = best;
    return true;
}

// floats of one batch group's partial: accumulator-native [gene block][4 HT x 2][64] float4, then dg [N], dbs [H], dbp [H]
size_t pp_adj3(const D1 &d) { return align_up((size_t)d.nblk * (4 * d.HT * 2 * 256) + d.N + 2 * d.H, 64); }

Regions make_layout3(const D1 &d, bool grads)
{
    LayoutSpec s;
    s.part_rows = s.zbuf_rows = (size_t)d.ntg * 4 * d.HT * 4 + d.ntg;   // hidden rows + norm rows per group
    s.two_sets = true;
    s.tail = true;
    s.pp = (long long)pp_adj3(d);
    s.nparts = d.TG;   // one partial per workgroup of a gene tile = per batch group (k1_solve_adj3: quad_accept)
    // every wave that owns a tile first-touches its whole partial (plain stores) in its first quadrature visit, or
    // zero-fills it at the end of the launch when its group never stepped
    s.dtheta = grads ? pp_adj3(d) * 4 * d.TG : 0;
    // transposed hidden rows of the seven ring slots, shared by a group's workgroups: [group][tile][7][4 HT][64] float4
    s.has_hq = true;
    s.hq = grads ? (size_t)d.TG * d.ntg * 7 * 4 * d.HT * 1024 : 0;
    return make_regions(d, s);
}

const void *prepare_adj3(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    pack_images(a, p, st);
    // HALF: the last hidden tile has at most 8 live rows (H <= 40 with three tiles; rho16 in phx_mfma_v3common.inc)
    const char *eh = getenv("PHX_V3_HALF");   // diagnostic: 0 = full last tile also where half of it is padding
    const bool half = p->H <= 16 * (d.HT - 1) + 8 && !(eh && eh[0] == '0');
    const bool split = v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1;   // small batch: the waves of a tile split its blocks
    return split ? (half ? reinterpret_cast<const void *>(k1_solve_adj3<3, true, true>)
                         : reinterpret_cast<const void *>(k1_solve_adj3<3, false, true>))
                 : (half ? reinterpret_cast<const void *>(k1_solve_adj3<3, true, false>)
                         : reinterpret_cast<const void *>(k1_solve_adj3<3, false, false>));
}

hipError_t launch_adj3(const void *fn, const SolveArgs &a, hipStream_t st)
{
    // PHX_PROF=2: + per-block timers of the sweeps, 3: + of the quadrature; 8: k3_tail_adj3 follows (reduce_adj3)
    const int flags = a.grads | (a.w.prof_level == 2 ? 2 : 0) | (a.w.prof_level == 3 ? 4 : 0) | (adj3_tail_on(a) ? 8 : 0);
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved,
                             a.grad_y, a.adj_y0, a.status, a.nfe, a.nsteps, flags, a.PP, (const int *)nullptr, 1);   // (no list)
}

bool reduce_adj3(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    const D1 &d = a.d;
    // the tail kernel: the visits the solve deferred + the sum over the groups, unconditionally (the workspace header says
    // which groups deferred: no host-side decision, so a captured step replays it as it is)
    if (adj3_tail_on(a)) return launch_adj3_tail(a, g, overwrite, st);
    const long long total = (long long)d.nblk * (4 * d.HT * 2 * 64) + d.N + 2 * d.H;
    hipLaunchKernelGGL((k3_reduce_grads<3>), dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, st, a.w.dtheta, npart,
                       a.PP, d.N, d.H, d.nblk, g->Ws, g->Wp, g->WaT, g->g, g->bs, g->bp, overwrite, g->Wa);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

namespace phxh {
// the launch k1_solve_adj3 takes, whatever the group size (plan_adj3 adds the choice against k1_solve_adj2)
bool plan_adj3_any(const Shape &s, D1 *out)
{
    if (s.cus <= 0 || s.calls > 1 || s.method != PHX_DOPRI5 || s.H > 48) return false;
    const Switches sw = read_switches(SW_ADJ | SW_V3_NB);
    if (sw.v0) return false;
    const int HT = 3;
    // (control LDS + that of the block-split combine where the batch is that small: v3_split_parts)
    return plan_resident(s, make_tiles(HT, 1, s.H, NVEC_ADJ3), 4, 0, sw.v3_nb,
                         [&](int NW, int TPW, int TG, int ntg, int Bt) {
                             return ((ctl3_bytes(Bt, ntg) + 15) & ~(size_t)15) +
                                    (v3_split_parts(TG, NW, TPW, ntg) > 1 ? v3_comb_bytes(NW, 4 * HT) : 0);
                         }, out);
}

const Backend &adj3_backend()
{
    static const Backend b = {3, true, false, true, plan_adj3, make_layout3, lds_bytes_adj3, plan6_ht, prepare_adj3,
                              launch_adj3, reduce_adj3};
    return b;
}
}  // namespace phxh
