// phx_adj2.hip -- translation unit of the second-generation adjoint kernel (k1_solve_adj2, phx_mfma_adj2.inc):
// launch planning, workspace layout and the host entry points the C ABI (phx_engine.hip) calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "phx_solver.hpp"
#include "phx_host.hpp"

using namespace phxh;

#include "phx_mfma_common.inc"
#include "phx_mfma_adj2.inc"
#include "phx_plan.hpp"

namespace {

size_t lds_bytes_adj2(const D1 &d) { return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + adj2_ctl_bytes(d.NW / 2, d.TPW); }

// picks (NP, TPW, NB): minimise the per-wave MFMA work TPW*NB subject to LDS and residency (one workgroup per CU).  Not a
// case of plan_resident: the slots of a workgroup are its wave PAIRS, the two forms are tried from the smaller one up and
// the cost knows the pairs.  Any method.
bool plan_adj2(const Shape &s, D1 *out)
{
    if (s.cus <= 0 || s.calls > 1 || s.H > 128) return false;
    const Switches sw = read_switches(SW_ADJ | SW_ADJ2);
    if (sw.v0 || sw.adj == 1) return false;
    const Tiles t = make_tiles(s.H <= 48 ? 3 : 8, 1, s.H, NVEC_ADJ2);
    const int nblk = (s.N + 31) / 32, ntt = (s.B + 15) / 16;
    long long best_cost = -1;
    D1 best{};
    // NP pairs per workgroup: 2 (four waves, one per SIMD, 512 registers each; a wave alternates between its TPW >= 2
    // tiles, so one tile's exchange is in flight while the other tile computes) or 4 (eight waves, 256 registers)
    // Measured on MI355X (profiles/r2_adjoint_variants.txt): wide hidden layers (HT = 8) want the 512-register
    // form (NP = 2: no spills), narrow ones (HT = 3) the eight-wave form (NP = 4); PHX_ADJ2_NP overrides (diagnostic)
    const int np_only = sw.adj2_np ? atoi(sw.adj2_np) : (t.HT == 8 ? 2 : 4);
    for (int NP = 2; NP <= 4; NP += 2)
    for (int TPW = 1; TPW <= 4; TPW <<= 1) {
        if (np_only && NP != np_only) continue;
        const int slots = NP * TPW, TG = (ntt + slots - 1) / slots;
        const int ntg = TG == 1 ? std::min(slots, ntt) : slots, Bt = 16 * ntg;
        if (s.control == PHX_CTRL_SHARED && TG != 1) continue;
        const size_t cb = adj2_ctl_bytes(NP, TPW);
        if (cb + t.blkbytes > LDS_BUDGET) continue;
        const int NBmax = (int)std::min<size_t>((LDS_BUDGET - cb) / t.blkbytes, 8);
        for (int NB = 1; NB <= NBmax; ++NB) {
            if ((long long)TG * ((nblk + NB - 1) / NB) > s.cus) continue;
            // per-SIMD MFMA work ~ TPW * NB * (waves per SIMD); at equal work one wave per SIMD with two tiles wins
            const long long cost = (long long)TPW * NB * (NP / 2) * 1000 + Bt / 4 + (NP == 2 && TPW >= 2 ? 0 : 40);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = make_d1(s, t, 2 * NP, TPW, NB, TG, ntg, false);
            }
            break;  // smallest feasible NB for this TPW is the cheapest
        }
    }
    if (best_cost < 0) return false;
    // Narrow hidden layer exchanged among many gene tiles (the breast-cancer shape: H = 40, 59 members per group): the
    // first-generation kernel (one wave per trajectory tile doing both halves of the augmented state: twice the MFMA
    // work per gene-block visit) is still the faster one there -- 0.73 against 0.90 ms.  PHX_ADJ=v2 forces this kernel.
    // (with a step size too: k1_solve_adj has the sub-step loop as well)
    if (best.HT == 3 && best.G > 32 && sw.adj != 2) return false;
    *out = best;
    return true;
}

// start delay of the second half of the wave pairs (100 MHz ticks); PHX_STAGGER_US overrides (diagnostic)
int prof_wave()
{
    if (const char *e = getenv("PHX_PROF_WAVE")) return atoi(e) & 7;
    return 0;
}
int stagger_ticks()
{
    if (const char *e = getenv("PHX_STAGGER_US")) return atoi(e) < 0 ? -1 : atoi(e) * 100;   // < 0: generic sweeps only
    return 0;
}


Regions make_layout2(const D1 &d, bool grads)
{
    LayoutSpec s;
    const size_t RH = (size_t)d.ntg * 4 * d.HT * 4;
    s.part_rows = RH + 2 * (size_t)d.ntg;   // partial rows per workgroup: hidden rows + one norm row per tile and side
    s.zbuf_rows = RH + 4 * (size_t)d.ntg;   // reduced rows per group: the norm rows are double buffered
    s.tail = true;
    s.pp = (long long)align_up((size_t)4 * d.H * d.N + d.N + 2 * d.H, 4);
    s.nparts = d.TG == 1 ? (d.ntg + d.TPW - 1) / d.TPW : d.TG * (d.NW / 2);   // pairs that own tiles
    // The quadrature first-touches every element of a pair's partial (plain stores) -- but only pairs that own at
    // least one real trajectory ever run it: with several groups the last group's trailing pairs can hold padding
    // tiles only (their controllers start "done"), with T < 2 nobody steps, and a pair whose trajectories all
    // failed at once never gets there either.  Every partial must read as zero then: always cleared (a few us).
    s.dtheta = grads ? (size_t)s.pp * 4 * d.TG * (d.NW / 2) : 0;
    s.has_hq = true;
    s.hq = grads ? (size_t)d.TG * d.G * d.NW * d.TPW * 7 * 2 * d.HT * 256 * 4 : 0;
    return make_regions(d, s);
}

const void *prepare_adj2(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    pack_images(a, p, st);
    if (d.HT == 3)
        return d.NW == 8 ? reinterpret_cast<const void *>(k1_solve_adj2<3, 4>) : reinterpret_cast<const void *>(k1_solve_adj2<3, 2>);
    return d.NW == 8 ? reinterpret_cast<const void *>(k1_solve_adj2<8, 4>) : reinterpret_cast<const void *>(k1_solve_adj2<8, 2>);
}

hipError_t launch_adj2(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_plain(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved, a.grad_y,
                        a.adj_y0, a.status, a.nfe, a.nsteps, a.grads, a.PP, stagger_ticks(), prof_wave());
}

bool reduce_adj2(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    return launch_reduce_grads(a.w.dtheta, npart, a.PP, a.d.N, a.d.H, g, overwrite, st);
}

}  // namespace

namespace phxh {
const Backend &adj2_backend()
{
    static const Backend b = {2, false, true, false, plan_adj2, make_layout2, lds_bytes_adj2, plan6_ht, prepare_adj2,
                              launch_adj2, reduce_adj2, true};
    return b;
}
}  // namespace phxh
