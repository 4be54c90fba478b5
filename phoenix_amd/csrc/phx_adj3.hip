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

namespace {

int adj3_mode()   // -1: disabled (another kernel forced), 1: forced for every shape it supports, 0: by shape
{
    if (force_v0()) return -1;
    const char *e = getenv("PHX_ADJ");
    if (!e) return 0;
    if (strcmp(e, "v3") == 0) return 1;
    if (strcmp(e, "v1") == 0 || strcmp(e, "v2") == 0) return -1;
    return 0;
}

// picks (NW, TPW, NB) like plan_v1 does for the first backward kernel: one wave per SIMD (the augmented sweeps need the
// 512-register budget), the smallest gene tile that keeps TG x G workgroups resident, the smallest batch group
bool plan_adj3(int N, int H, int B, int T, int control, int method, D1 *out)
{
    const int cus = num_cus();
    const int mode = adj3_mode();
    if (cus <= 0 || mode < 0 || method != PHX_DOPRI5 || H > 48) return false;
    const int HT = 3;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, H) * 4;
    const int nblk = (N + 31) / 32, ntt = (B + 15) / 16;
    long long best_cost = -1;
    D1 best{};
    for (int NW = 4; NW >= 1; NW >>= 1)
        for (int TPW = 1; TPW <= 4; TPW <<= 1) {
            const int slots = NW * TPW, TG = (ntt + slots - 1) / slots;
            const int ntg = TG == 1 ? std::min(slots, ntt) : slots, Bt = 16 * ntg;
            const bool helpers = ntg < slots;
            if (control == PHX_CTRL_SHARED && TG != 1) continue;
            // (+ the LDS of the block-split combine where the batch is that small: v3_split_parts)
            const size_t cb = ((ctl3_bytes(Bt, ntg) + 15) & ~(size_t)15) +
                              (v3_split_parts(TG, NW, TPW, ntg) > 1 ? v3_comb_bytes(NW, 4 * HT) : 0);
            if (cb + blkbytes > LDS_BUDGET) continue;
            const int NBmax = (int)std::min<size_t>((LDS_BUDGET - cb) / blkbytes, 8);
            const char *enb = getenv("PHX_V3_NB");   // experiment: smallest gene tile to consider
            for (int NB = enb ? std::max(1, atoi(enb)) : 1; NB <= NBmax; ++NB) {
                const int G = (nblk + NB - 1) / NB;
                if ((long long)TG * G > cus) continue;
                const long long cost = (long long)TPW * NB * 1000 + Bt / 4 - (helpers && TPW == 1 ? 50 : 0);
                if (best_cost < 0 || cost < best_cost) {
                    best_cost = cost;
                    best.N = N; best.H = H; best.B = B; best.T = T; best.HT = HT; best.NB = NB; best.NW = NW;
                    best.TPW = TPW; best.G = G; best.TG = TG; best.nblk = nblk; best.ntg = ntg; best.Bt = Bt;
                    best.nvec = NVEC_ADJ3; best.BN = (long long)B * N; best.HC = 1; best.Hc = H;
                    best.Bcall = 0; best.cntN = (long long)B * N;
                }
                break;  // smallest feasible NB for this (NW, TPW) is the cheapest
            }
        }
    if (best_cost < 0) return false;
    // by shape: the many-member exchange of a narrow hidden layer (the breast-cancer shape) is this kernel's; groups of
    // up to 32 gene tiles stay with the wave-pair kernel (k1_solve_adj2), which is faster there.  PHX_ADJ=v3 forces it.
    if (mode == 0 && best.G <= 32) return false;
    *out = best;
    return true;
}

// floats of one batch group's partial: accumulator-native [gene block][4 HT x 2][64] float4, then dg [N], dbs [H], dbp [H]
size_t pp_adj3(const D1 &d) { return align_up((size_t)d.nblk * (4 * d.HT * 2 * 256) + d.N + 2 * d.H, 64); }


Regions make_layout3(const D1 &d, bool grads)
{
    Regions L{};
    Take take;
    const size_t R = (size_t)d.ntg * 4 * d.HT * 4 + d.ntg;   // hidden rows + norm rows per group
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * R * 64 * 8);
    L.xbytes = take.off - L.part;                            // header + set 0: what a fill covers (phx_mfma_v3common.inc: XSet)
    L.part1 = take((size_t)d.TG * d.G * R * 64 * 8);         // set 1: cleaned by the launch that works in set 0
    L.zbuf1 = take((size_t)d.TG * R * 64 * 8);
    L.scratch = take((size_t)d.TG * d.G * NVEC_ADJ3 * d.ntg * d.NB * 512 * 4);
    L.pp = (long long)pp_adj3(d);
    L.nparts = d.TG;   // one partial per workgroup of a gene tile = per batch group (k1_solve_adj3: quad_accept)
    // every wave that owns a tile first-touches its whole partial (plain stores) in its first quadrature visit, or
    // zero-fills it at the end of the launch when its group never stepped
    L.dtheta = take(grads ? pp_adj3(d) * 4 * d.TG : 0);
    L.prof = take((size_t)d.TG * d.G * 16 * 8);
    L.wimg = take((size_t)d.nblk * blk_floats_ch(d.HT, d.H) * 4);
    // transposed hidden rows of the seven ring slots, shared by a group's workgroups: [group][tile][7][4 HT][64] float4
    L.hq = take(grads ? (size_t)d.TG * d.ntg * 7 * 4 * d.HT * 1024 : 0);
    L.total = take.off;
    return L;
}

size_t lds_bytes_adj3(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + ((ctl3_bytes(d.Bt, d.ntg) + 15) & ~(size_t)15) +
           (v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1 ? v3_comb_bytes(d.NW, 4 * d.HT) : 0);
}

const void *prepare_adj3(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    if (p->wimg) a.w.wimg = (const float *)p->wimg;   // packed once by the caller for these parameter values
    else
        hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, 1, p->H,
                           blk_floats_ch(d.HT, p->H));
    a.lds = lds_bytes_adj3(d);
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
    // PHX_PROF=2: + per-block timers of the sweeps, 3: + of the quadrature
    const int flags = a.grads | (a.w.prof_level == 2 ? 2 : 0) | (a.w.prof_level == 3 ? 4 : 0);
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved,
                             a.grad_y, a.adj_y0, a.status, a.nfe, a.nsteps, flags, a.PP);
}

bool reduce_adj3(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    const D1 &d = a.d;
    const long long total = (long long)d.nblk * (4 * d.HT * 2 * 64) + d.N + 2 * d.H;
    hipLaunchKernelGGL((k3_reduce_grads<3>), dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, st, a.w.dtheta, npart,
                       a.PP, d.N, d.H, d.nblk, g->Ws, g->Wp, g->WaT, g->g, g->bs, g->bp, overwrite, g->Wa);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

namespace phxh {
const Backend &adj3_backend()
{
    static const Backend b = {3, true, false, true, plan_adj3, make_layout3, plan6_ht, prepare_adj3, launch_adj3, reduce_adj3};
    return b;
}
}  // namespace phxh
