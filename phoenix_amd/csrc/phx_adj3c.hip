// phx_adj3c.hip -- translation unit of the third-generation backward kernel for wide hidden layers (k1_solve_adj3c,
// phx_mfma_adj3c.inc: hidden chunks of <= 48 rows): launch planning, workspace layout and the host entry points the C ABI
// (phx_engine.hip) calls.
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
#include "phx_mfma_adj3c.inc"
#include "phx_plan.hpp"

namespace {

// plan_chunked with the backward kernel's rules.  At most FOUR (tile, block) slots per wave: the eight-slot instantiation
// needs more than the 512 registers (3 460 spilled, and this compiler fails on its <8, false> form); a batch that needs
// more slots runs as several launches (pick_chunk)
bool plan_adj3c(const Shape &s, D1 *out)
{
    if (!chunked_shape(s)) return false;
    const Switches sw = read_switches(SW_ADJ | SW_CHUNKED);
    if (sw.v0 || sw.adj == 1 || sw.adj == 2 || sw.v3c_off) return false;
    return plan_chunked(s, sw, ChunkedRules{NVEC_ADJ3C, sw.v3c_slots, 4, false, HSA_BYTES}, ctl3c_bytes,
                        [](int Bt, int ntg, int parts) { return hsa_offset(Bt, ntg) + spa_bytes(ntg, parts); }, out);
}

// floats of one batch group's partial: accumulator-native [gene block][chunk][4 HT x 2][64] float4, then dg [N], dbs [H], dbp [H]
size_t pp_adj3c(const D1 &d) { return align_up((size_t)d.nblk * d.HC * (4 * d.HT * 2 * 256) + d.N + 2 * d.H, 64); }

Regions make_layout3c(const D1 &d, bool grads)
{
    LayoutSpec s;
    s.part_rows = s.zbuf_rows = (size_t)d.ntg * d.HC * 4 * d.HT * 4 + d.ntg;   // hidden rows of every chunk + norm rows per group
    s.two_sets = true;
    s.tail = true;
    s.pp = (long long)pp_adj3c(d);
    s.nparts = d.TG;   // one partial per batch group (the quadrature's items: every slot has one owner wave)
    // every item's owner first-touches its slots (plain stores) in the first quadrature visit, or zero-fills them at the
    // end of the launch when its group never stepped
    s.dtheta = grads ? pp_adj3c(d) * 4 * d.TG : 0;
    // transposed hidden rows of the seven ring slots, shared by a group's workgroups: [group][tile][7][chunk][4 HT][64] float4
    s.has_hq = true;
    s.hq = grads ? (size_t)d.TG * d.ntg * 7 * d.HC * 4 * d.HT * 1024 : 0;
    return make_regions(d, s);
}

size_t lds_bytes_adj3c(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.Hc) * 4 * d.NB * (d.res ? d.HC : 1) +
           (d.hb ? hsa_offset(d.Bt, d.ntg) + HSA_BYTES
                 : (d.split > 1 ? hsa_offset(d.Bt, d.ntg) + spa_bytes(d.ntg, d.split) : ctl3c_bytes(d.Bt, d.ntg)));
}

const void *prepare_adj3c(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    // the chunk images of this kernel family are not the caller's phx_params.wimg format for H > 48: packed per launch
    pack_images(a, p, st, false);
    const int nbt = d.TPW * d.NB <= 1 || d.split > 1 ? 1 : 4;   // (tile, block) slots per wave the kernel is built for
    const bool half = d.Hc <= 40;   // every chunk's last tile has at most 8 live rows (rho16, phx_mfma_v3common.inc)
    switch (nbt * 2 + (half ? 1 : 0) + (d.hb ? 32 : 0)) {
    case 35: return reinterpret_cast<const void *>(k1_solve_adj3c<1, true, true>);
    case 34: return reinterpret_cast<const void *>(k1_solve_adj3c<1, false, true>);
    case 3: return reinterpret_cast<const void *>(k1_solve_adj3c<1, true, false>);
    case 2: return reinterpret_cast<const void *>(k1_solve_adj3c<1, false, false>);
    case 9: return reinterpret_cast<const void *>(k1_solve_adj3c<4, true, false>);
    case 8: return reinterpret_cast<const void *>(k1_solve_adj3c<4, false, false>);
    default: return nullptr;
    }
}

hipError_t launch_adj3c(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved,
                             a.grad_y, a.adj_y0, a.status, a.nfe, a.nsteps, a.grads, a.PP);
}

bool reduce_adj3c(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    const D1 &d = a.d;
    const long long total = (long long)d.nblk * d.HC * (4 * d.HT * 2 * 64) + d.N + 2 * d.H;
    hipLaunchKernelGGL(k3c_reduce_grads, dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, st, a.w.dtheta, npart, a.PP,
                       d.N, d.H, d.nblk, d.HC, d.Hc, g->Ws, g->Wp, g->WaT, g->g, g->bs, g->bp, overwrite, g->Wa);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

namespace phxh {
const Backend &adj3c_backend()
{
    static const Backend b = {4, true, false, true,
                                    plan_adj3c, make_layout3c, lds_bytes_adj3c, plan6_chunked, prepare_adj3c, launch_adj3c, reduce_adj3c};
    return b;
}
}  // namespace phxh
