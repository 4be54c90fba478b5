// phx_fwd3c.hip -- translation unit of the third-generation forward solve for wide hidden layers (k1_solve_fwd3c,
// phx_mfma_fwd3c.inc: hidden chunks of <= 48 rows): launch planning, workspace layout and the host entry points the C ABI
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
#include "phx_mfma_fwd3c.inc"

namespace {

bool fwd3c_disabled()
{
    const char *e = getenv("PHX_FWD");   // diagnostic: PHX_FWD=v1 keeps every forward solve on k1_solve_fwd
    const char *c = getenv("PHX_V3C");   // diagnostic: PHX_V3C=0 switches the chunked third-generation kernels off
    return force_v0() || (e && strcmp(e, "v1") == 0) || (c && c[0] == '0');
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Hidden chunks: HC = ceil(H / 48) chunks of Hc = ceil(H / HC) rows, three 16-row tiles each (120 -> 3 x 40, 200 -> 5 x 40).
// (NW, TPW, NB): one wave per SIMD, gene tiles of 1 / 2 / 4 / 8 blocks, at most 8 (tile, block) slots per wave (the kernel
// keeps their partial sums in registers); all chunks LDS resident when they fit, else one re-staged slot.  Cost: the
// per-wave MFMA work first, then the exchange volume (members per group).  A plan of ONE slot per wave whose workgroups
// leave half the chip idle takes HALF-BLOCK gene tiles (hb: twice the workgroups, half the sweep work each).
// calls > 1 (shared control): B = calls x Bcall rows, one batch group per call (plan_v1's rule: D1::Bcall)
bool plan_fwd3c_cus(int cus, int N, int H, int B, int T, int control, int method, int calls, D1 *out)
{
    if (cus <= 0 || fwd3c_disabled() || method != PHX_DOPRI5 || H <= 48 || H > 256) return false;
    if (calls > 1 && (control != PHX_CTRL_SHARED || B % calls != 0)) return false;
    const int Bcall = calls > 1 ? B / calls : 0;
    const int HT = 3, HC = (H + 47) / 48, Hc = (H + HC - 1) / HC;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, Hc) * 4;
    const int nblk = (N + 31) / 32, ntt = ((Bcall ? Bcall : B) + 15) / 16;
    const int fnb = env_int("PHX_V3C_NB", 0), ftpw = env_int("PHX_V3C_TPW", 0), fres = env_int("PHX_V3C_RES", -1);
    const int fhb = env_int("PHX_V3C_HB", -1);
    long long best_cost = -1;
    D1 best{};
    for (int NW = 4; NW >= 1; NW >>= 1)
        for (int TPW = 1; TPW <= 8; TPW <<= 1) {
            if (ftpw > 0 && TPW != ftpw) continue;
            const int slots = NW * TPW;
            int TG = (ntt + slots - 1) / slots;
            int ntg = TG == 1 ? std::min(slots, ntt) : slots;
            // More batch groups of FEWER trajectory tiles where the chip has room for them (one tile per wave plans, twice
            // the gene blocks -- half-block tiles -- still resident): the groups' exchanges carry fewer rows and a tile gets
            // helper waves (measured, round 5: -8 ... -32 % of a launch; 23 yeast pairs as two groups of one tile: neutral).
            // PHX_V3C_NTG forces the tiles per group (4: the plan before this rule).
            const int fntg = env_int("PHX_V3C_NTG", 0);
            if (Bcall) {   // a call is one group
                if (slots < ntt) continue;
                TG = calls; ntg = ntt;
            } else if (fntg > 0 && fntg <= slots) { ntg = std::min(fntg, ntt); TG = (ntt + ntg - 1) / ntg; }
            else if (fntg == 0 && TPW == 1 && control != PHX_CTRL_SHARED) {
                // (one-tile groups may take three quarters of the chip, two-tile groups half of it: beyond, the forward
                // launch measured +8 ... +18 % -- 252 half-block workgroups at two tiles per group -- where the backward gains)
                for (int c = 1; c < ntg; c <<= 1) {
                    const int tgc = (ntt + c - 1) / c;
                    if ((long long)tgc * nblk * 2 * 4 <= (long long)cus * (c == 1 ? 3 : 2)) { ntg = c; TG = tgc; break; }
                }
            }
            const int Bt = 16 * ntg;
            // the controllers step one trajectory per thread (k1_solve_fwd3c: `tid < Bt`): a group of more trajectories
            // than the workgroup has threads (eight-tile waves, more than 16 tiles) would leave the rest unsolved
            if (Bt > 64 * NW) continue;
            const bool helpers = ntg < slots;
            if (control == PHX_CTRL_SHARED && TG != 1 && !Bcall) continue;
            const size_t cb = ctlf3c_bytes(Bt, ntg);
            for (int NB = 1; NB <= 8 && TPW * NB <= 8; NB <<= 1) {
                if (fnb > 0 && NB != fnb) continue;
                if (cb + blkbytes * NB > LDS_BUDGET) break;
                const int G = (nblk + NB - 1) / NB;
                if ((long long)TG * G > cus) continue;
                bool res = cb + blkbytes * NB * HC <= LDS_BUDGET;
                if (fres == 0) res = false;
                const long long cost = (long long)TPW * NB * 1000 + (res ? 0 : 150) + G - (helpers && TPW == 1 ? 50 : 0);
                if (best_cost < 0 || cost < best_cost) {
                    best_cost = cost;
                    best.N = N; best.H = H; best.B = B; best.T = T; best.HT = HT; best.NB = NB; best.NW = NW;
                    best.TPW = TPW; best.G = G; best.TG = TG; best.nblk = nblk; best.ntg = ntg; best.Bt = Bt;
                    best.nvec = NVEC_FWD3C; best.BN = (long long)B * N; best.HC = HC; best.Hc = Hc;
                    best.Bcall = Bcall; best.cntN = (long long)(Bcall ? Bcall : B) * N; best.res = res ? 1 : 0;
                    const int nslot = TPW * NB;
                    // measured (round 5, H = 120 / 200, 8..220 gene blocks, 16..128 trajectories): -9..-33 % of a launch while
                    // the groups' rows times their workgroups stay small (four-tile groups on at most half the chip, one-tile
                    // groups on all of it) and a group has at most 160 members; +5..+24 % beyond (tools/v3c_check.py hbgrid)
                    const bool hb_fits = nslot == 1 && res && (long long)TG * G * 2 <= cus && cb + HSF_BYTES + 16 + blkbytes * HC <= LDS_BUDGET;
                    best.hb = (hb_fits && fhb != 0 && (fhb == 1 || ((long long)TG * G * ntg <= cus && 2 * nblk <= 160))) ? 1 : 0;
                    // block split: a tile's gene blocks on the workgroup's spare waves (small batches of multi-block tiles)
                    best.split = 1;
                    if (!best.hb && TPW == 1 && NB > 1 && ntg * NB <= NW && env_int("PHX_V3C_SPLIT", 1) != 0) {
                        const int parts = std::min(NW / ntg, NB);
                        if (hsf_offset(Bt, ntg) + spf_bytes(ntg, parts) + blkbytes * NB * (res ? HC : 1) <= LDS_BUDGET)
                            best.split = parts;
                    }
                }
            }
        }
    if (best_cost < 0) return false;
    if (best.hb) best.G = 2 * best.nblk;
    *out = best;
    return true;
}

bool plan_fwd3c(int N, int H, int B, int T, int control, int method, D1 *out)
{
    return plan_fwd3c_cus(num_cus(), N, H, B, T, control, method, 1, out);
}


Regions make_layout_f3c(const D1 &d, bool)
{
    Regions L{};
    Take take;
    const size_t R = (size_t)d.ntg * d.HC * 2 * d.HT * 4 + d.ntg;   // hidden rows of every chunk + norm rows per group
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * R * 64 * 8);
    L.xbytes = take.off - L.part;                            // header + set 0: what a fill covers (phx_mfma_v3common.inc: XSet)
    L.part1 = take((size_t)d.TG * d.G * R * 64 * 8);         // set 1: cleaned by the launch that works in set 0
    L.zbuf1 = take((size_t)d.TG * R * 64 * 8);
    L.scratch = take((size_t)d.TG * d.G * NVEC_FWD3C * d.ntg * d.NB * 512 * 4);
    L.prof = take((size_t)d.TG * d.G * 16 * 8);
    L.wimg = take((size_t)d.nblk * d.HC * blk_floats_ch(d.HT, d.Hc) * 4);
    L.total = take.off;
    return L;
}

size_t lds_bytes_fwd3c(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.Hc) * 4 * d.NB * (d.res ? d.HC : 1) +
           (d.hb ? hsf_offset(d.Bt, d.ntg) + HSF_BYTES
                 : (d.split > 1 ? hsf_offset(d.Bt, d.ntg) + spf_bytes(d.ntg, d.split) : ctlf3c_bytes(d.Bt, d.ntg)));
}

const void *prepare_fwd3c(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    // the chunk images of this kernel family (three-tile chunks) are not the caller's phx_params.wimg format for H > 48
    // (one eight-tile chunk / seven-tile 100-row chunks): packed per launch from the parameter tensors
    hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk * d.HC), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, d.HC, d.Hc,
                       blk_floats_ch(d.HT, d.Hc));
    a.lds = lds_bytes_fwd3c(d);
    // (tile, block) slots per wave the kernel is built for (unused slots of the eight-slot form cost a scalar branch each)
    const int nbt = d.TPW * d.NB <= 1 || d.split > 1 ? 1 : 8;
    const bool half = d.Hc <= 40;   // every chunk's last tile has at most 8 live rows (rho16, phx_mfma_v3common.inc)
    if (d.Bcall > 0)   // several calls, a time row each (one call alone is an ordinary shared-control launch)
        switch (nbt * 2 + (half ? 1 : 0) + (d.hb ? 32 : 0)) {
        case 35: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, true, true>);
        case 34: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, true, true>);
        case 3: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, false, true>);
        case 2: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, false, true>);
        case 17: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, true, false, true>);
        default: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, false, false, true>);
        }
    switch (nbt * 2 + (half ? 1 : 0) + (d.hb ? 32 : 0)) {
    case 35: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, true>);
    case 34: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, true>);
    case 3: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, false>);
    case 2: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, false>);
    case 17: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, true, false>);
    default: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, false, false>);
    }
}

hipError_t launch_fwd3c(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.y0, a.t, a.sol,
                             a.status, a.nfe, a.nsteps);
}

}  // namespace

namespace phxh {
const Backend &fwd3c_backend()
{
    static const Backend b = {4, true, false, true,
                                    plan_fwd3c, make_layout_f3c, plan6_chunked, prepare_fwd3c, launch_fwd3c, nullptr};
    return b;
}
bool plan_fwd3c_calls(int cus, int N, int H, int Bcall, int calls, int T, D1 *out)
{
    return plan_fwd3c_cus(cus, N, H, Bcall * calls, T, PHX_CTRL_SHARED, PHX_DOPRI5, calls, out);
}
}  // namespace phxh
