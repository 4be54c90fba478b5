// phx_fwd3.hip -- translation unit of the third-generation forward solve (k1_solve_fwd3, phx_mfma_fwd3.inc): launch
// planning, workspace layout and the host entry points the C ABI (phx_engine.hip) calls.
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
#include "phx_mfma_fwd3.inc"

namespace {

bool fwd3_disabled()
{
    const char *e = getenv("PHX_FWD");   // diagnostic: PHX_FWD=v1 keeps every forward solve on k1_solve_fwd
    return force_v0() || (e && strcmp(e, "v1") == 0);
}

// (NW, TPW, NB) as plan_v1 picks them for the forward kernel: per-SIMD MFMA work first, then two waves per SIMD, then
// the smallest batch group
// calls > 1 (shared control): B = calls x Bcall rows, one batch group per call (plan_v1's rule: D1::Bcall)
bool plan_fwd3_cus(int cus, int N, int H, int B, int T, int control, int method, int calls, D1 *out)
{
    if (cus <= 0 || fwd3_disabled() || method != PHX_DOPRI5 || H > 48) return false;
    if (calls > 1 && (control != PHX_CTRL_SHARED || B % calls != 0)) return false;
    const int Bcall = calls > 1 ? B / calls : 0;
    const int HT = 3;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, H) * 4;
    const int nblk = (N + 31) / 32, ntt = ((Bcall ? Bcall : B) + 15) / 16;
    long long best_cost = -1;
    D1 best{};
    // One wave per SIMD (NW <= 4).  The eight-wave form (two waves per SIMD under a 256-register cap) computed wrong step
    // sizes in round 3 -- the store-data hazard of phx_mfma_v3common.inc, not the form itself: rebuilt in round 4 with the
    // guarded stores it passes the parity suite, and it is no faster at C4 (0.266-0.268 ms against 0.268-0.270: 38-148
    // spilled registers, twice the exchange members per group), so it is not built.
    int nwmax = 4;
    if (const char *e = getenv("PHX_V1_MAXNW")) nwmax = std::min(nwmax, std::max(1, atoi(e)));
    for (int NW = nwmax; NW >= 1; NW >>= 1)
        for (int TPW = 1; TPW <= 4; TPW <<= 1) {
            const int slots = NW * TPW, TG = Bcall ? calls : (ntt + slots - 1) / slots;
            if (Bcall && slots < ntt) continue;   // a call is one group
            const int ntg = (TG == 1 || Bcall) ? std::min(slots, ntt) : slots, Bt = 16 * ntg;
            const bool helpers = ntg < slots;
            if (control == PHX_CTRL_SHARED && TG != 1 && !Bcall) continue;
            // (+ the LDS of the block-split combine where the batch is that small: v3_split_parts)
            const size_t cb = ((ctlf3_bytes(Bt, ntg) + 15) & ~(size_t)15) +
                              (v3_split_parts(TG, NW, TPW, ntg) > 1 ? v3_comb_bytes(NW, 2 * HT) : 0);
            if (cb + blkbytes > LDS_BUDGET) continue;
            const int NBmax = (int)std::min<size_t>((LDS_BUDGET - cb) / blkbytes, 8);
            const char *enb = getenv("PHX_V3_NB");   // experiment: smallest gene tile to consider
            for (int NB = enb ? std::max(1, atoi(enb)) : 1; NB <= NBmax; ++NB) {
                const int G = (nblk + NB - 1) / NB;
                if ((long long)TG * G > cus) continue;
                const long long cost = (long long)TPW * NB * ((NW + 3) / 4) * 1000 + (4 - NW) * 100 + Bt / 4 -
                                       (helpers && TPW == 1 ? 50 : 0);
                if (best_cost < 0 || cost < best_cost) {
                    best_cost = cost;
                    best.N = N; best.H = H; best.B = B; best.T = T; best.HT = HT; best.NB = NB; best.NW = NW;
                    best.TPW = TPW; best.G = G; best.TG = TG; best.nblk = nblk; best.ntg = ntg; best.Bt = Bt;
                    best.nvec = NVEC_FWD3; best.BN = (long long)B * N; best.HC = 1; best.Hc = H;
                    best.Bcall = Bcall; best.cntN = (long long)(Bcall ? Bcall : B) * N;
                }
                break;  // smallest feasible NB for this (NW, TPW) is the cheapest
            }
        }
    if (best_cost < 0) return false;
    *out = best;
    return true;
}

bool plan_fwd3(int N, int H, int B, int T, int control, int method, D1 *out)
{
    return plan_fwd3_cus(num_cus(), N, H, B, T, control, method, 1, out);
}

Regions make_layout_f3(const D1 &d, bool)
{
    Regions L{};
    Take take;
    const size_t R = (size_t)d.ntg * 2 * d.HT * 4 + d.ntg;   // hidden rows + norm rows per group
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * R * 64 * 8);
    L.xbytes = take.off - L.part;                            // header + set 0: what a fill covers (phx_mfma_v3common.inc: XSet)
    L.part1 = take((size_t)d.TG * d.G * R * 64 * 8);         // set 1: cleaned by the launch that works in set 0
    L.zbuf1 = take((size_t)d.TG * R * 64 * 8);
    L.scratch = take((size_t)d.TG * d.G * NVEC_FWD3 * d.ntg * d.NB * 512 * 4);
    L.prof = take((size_t)d.TG * d.G * 16 * 8);
    L.wimg = take((size_t)d.nblk * blk_floats_ch(d.HT, d.H) * 4);
    L.total = take.off;
    return L;
}

size_t lds_bytes_fwd3(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + ((ctlf3_bytes(d.Bt, d.ntg) + 15) & ~(size_t)15) +
           (v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1 ? v3_comb_bytes(d.NW, 2 * d.HT) : 0);
}

const void *prepare_fwd3(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    if (p->wimg) a.w.wimg = (const float *)p->wimg;   // packed once by the caller for these parameter values
    else
        hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, 1, p->H,
                           blk_floats_ch(d.HT, p->H));
    a.lds = lds_bytes_fwd3(d);
    // HALF: the last hidden tile has at most 8 live rows (H <= 40 with three tiles; rho16 in phx_mfma_v3common.inc)
    const char *eh = getenv("PHX_V3_HALF");   // diagnostic: 0 = full last tile also where half of it is padding
    const bool half = p->H <= 16 * (d.HT - 1) + 8 && !(eh && eh[0] == '0');
    const char *et = getenv("PHX_V3_TERM");   // diagnostic: 0 = no terminal tiles, every step ends with the accept pass
    a.w.prof_level = (a.w.prof_level & 0xff) | ((et && et[0] == '0') ? FWD3_NO_TERM : 0);
    const bool split = v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1;   // small batch: the waves of a tile split its blocks
    if (d.Bcall > 0)   // several calls, a time row each (one call alone is an ordinary shared-control launch)
        return half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false, true>)
                    : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false, true>);
    return split ? (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, true>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, true>))
                 : (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false>));
}

hipError_t launch_fwd3(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.y0, a.t, a.sol,
                             a.status, a.nfe, a.nsteps);
}

}  // namespace

namespace phxh {
const Backend &fwd3_backend()
{
    static const Backend b = {3, true, false, true, plan_fwd3, make_layout_f3, plan6_ht, prepare_fwd3, launch_fwd3, nullptr};
    return b;
}
bool plan_fwd3_calls(int cus, int N, int H, int Bcall, int calls, int T, D1 *out)
{
    return plan_fwd3_cus(cus, N, H, Bcall * calls, T, PHX_CTRL_SHARED, PHX_DOPRI5, calls, out);
}
}  // namespace phxh
