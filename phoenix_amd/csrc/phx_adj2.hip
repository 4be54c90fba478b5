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

namespace {

bool adj2_disabled()
{
    const char *e = getenv("PHX_ADJ");
    return force_v0() || (e && strcmp(e, "v1") == 0);
}
bool adj2_forced()
{
    const char *e = getenv("PHX_ADJ");
    return e && strcmp(e, "v2") == 0;
}

// picks (TPW, NB): minimise the per-wave MFMA work TPW*NB subject to LDS and residency (one workgroup per CU)
bool plan_adj2(int N, int H, int B, int T, int control, int /* method: any */, D1 *out)
{
    const int cus = num_cus();
    if (cus <= 0 || H > 128 || adj2_disabled()) return false;
    const int HT = H <= 48 ? 3 : 8;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, H) * 4;
    const int nblk = (N + 31) / 32, ntt = (B + 15) / 16;
    long long best_cost = -1;
    D1 best{};
    // NP pairs per workgroup: 2 (four waves, one per SIMD, 512 registers each; a wave alternates between its TPW >= 2
    // tiles, so one tile's exchange is in flight while the other tile computes) or 4 (eight waves, 256 registers)
    // Measured on MI355X (profiles/r2_adjoint_variants.txt): wide hidden layers (HT = 8) want the 512-register
    // form (NP = 2: no spills), narrow ones (HT = 3) the eight-wave form (NP = 4); PHX_ADJ2_NP overrides (diagnostic)
    int np_only = HT == 8 ? 2 : 4;
    if (const char *e = getenv("PHX_ADJ2_NP")) np_only = atoi(e);
    for (int NP = 2; NP <= 4; NP += 2)
    for (int TPW = 1; TPW <= 4; TPW <<= 1) {
        if (np_only && NP != np_only) continue;
        const int slots = NP * TPW, TG = (ntt + slots - 1) / slots;
        const int ntg = TG == 1 ? std::min(slots, ntt) : slots, Bt = 16 * ntg;
        if (control == PHX_CTRL_SHARED && TG != 1) continue;
        const size_t cb = adj2_ctl_bytes(NP, TPW);
        if (cb + blkbytes > LDS_BUDGET) continue;
        const int NBmax = (int)std::min<size_t>((LDS_BUDGET - cb) / blkbytes, 8);
        for (int NB = 1; NB <= NBmax; ++NB) {
            const int G = (nblk + NB - 1) / NB;
            if ((long long)TG * G > cus) continue;
            // per-SIMD MFMA work ~ TPW * NB * (waves per SIMD); at equal work one wave per SIMD with two tiles wins
            const long long cost = (long long)TPW * NB * (NP / 2) * 1000 + Bt / 4 + (NP == 2 && TPW >= 2 ? 0 : 40);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best.N = N; best.H = H; best.B = B; best.T = T; best.HT = HT; best.NB = NB; best.NW = 2 * NP;
                best.TPW = TPW; best.G = G; best.TG = TG; best.nblk = nblk; best.ntg = ntg; best.Bt = Bt;
                best.nvec = NVEC_ADJ2; best.BN = (long long)B * N; best.HC = 1; best.Hc = H;
            }
            break;  // smallest feasible NB for this TPW is the cheapest
        }
    }
    if (best_cost < 0) return false;
    // Narrow hidden layer exchanged among many gene tiles (the breast-cancer shape: H = 40, 59 members per group): the
    // first-generation kernel (one wave per trajectory tile doing both halves of the augmented state: twice the MFMA
    // work per gene-block visit) is still the faster one there -- 0.73 against 0.90 ms.  PHX_ADJ=v2 forces this kernel.
    // (with a step size too: k1_solve_adj has the sub-step loop as well)
    if (best.HT == 3 && best.G > 32 && !adj2_forced()) return false;
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
    Regions L{};
    Take take;
    const size_t RH = (size_t)d.ntg * 4 * d.HT * 4;
    const size_t R = RH + 2 * (size_t)d.ntg;    // partial rows per workgroup: hidden rows + one norm row per tile and side
    const size_t RZ = RH + 4 * (size_t)d.ntg;   // reduced rows per group: the norm rows are double buffered
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * RZ * 64 * 8);
    L.xbytes = take.off - L.part;                           // granule buffers are zeroed before every launch
    L.scratch = take((size_t)d.TG * d.G * NVEC_ADJ2 * d.ntg * d.NB * 512 * 4);
    L.pp = (long long)align_up((size_t)4 * d.H * d.N + d.N + 2 * d.H, 4);
    L.nparts = d.TG == 1 ? (d.ntg + d.TPW - 1) / d.TPW : d.TG * (d.NW / 2);   // pairs that own tiles
    // The quadrature first-touches every element of a pair's partial (plain stores) -- but only pairs that own at
    // least one real trajectory ever run it: with several groups the last group's trailing pairs can hold padding
    // tiles only (their controllers start "done"), with T < 2 nobody steps, and a pair whose trajectories all
    // failed at once never gets there either.  Every partial must read as zero then: always cleared (a few us).
    L.dtheta = take(grads ? (size_t)L.pp * 4 * d.TG * (d.NW / 2) : 0);
    L.prof = take((size_t)d.TG * d.G * 16 * 8);
    L.wimg = take((size_t)d.nblk * blk_floats_ch(d.HT, d.H) * 4);
    L.hq = take(grads ? (size_t)d.TG * d.G * d.NW * d.TPW * 7 * 2 * d.HT * 256 * 4 : 0);
    L.total = take.off;
    return L;
}

const void *prepare_adj2(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    if (p->wimg) a.w.wimg = (const float *)p->wimg;   // packed once by the caller for these parameter values
    else
        hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, 1, p->H,
                           blk_floats_ch(d.HT, p->H));
    a.lds = (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + adj2_ctl_bytes(d.NW / 2, d.TPW);
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
    static const Backend b = {2, false, true, false, plan_adj2, make_layout2, plan6_ht, prepare_adj2, launch_adj2, reduce_adj2, true};
    return b;
}
}  // namespace phxh
