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

namespace {

bool adj3c_disabled()
{
    if (force_v0()) return true;
    const char *e = getenv("PHX_ADJ");   // another backward kernel forced
    if (e && (strcmp(e, "v1") == 0 || strcmp(e, "v2") == 0)) return true;
    const char *c = getenv("PHX_V3C");   // diagnostic: PHX_V3C=0 switches the chunked third-generation kernels off
    return c && c[0] == '0';
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// as plan_fwd3c (phx_fwd3c.hip): HC = ceil(H / 48) chunks of Hc = ceil(H / HC) rows; (NW, TPW, NB) with NB in {1, 2, 4, 8} and at
// most `maxslots` (tile, block) slots per wave
bool plan_adj3c(int N, int H, int B, int T, int control, int method, D1 *out)
{
    const int cus = num_cus();
    if (cus <= 0 || adj3c_disabled() || method != PHX_DOPRI5 || H <= 48 || H > 256) return false;
    const int HT = 3, HC = (H + 47) / 48, Hc = (H + HC - 1) / HC;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, Hc) * 4;
    const int nblk = (N + 31) / 32, ntt = (B + 15) / 16;
    const int fnb = env_int("PHX_V3C_NB", 0), ftpw = env_int("PHX_V3C_TPW", 0), fres = env_int("PHX_V3C_RES", -1);
    const int fhb = env_int("PHX_V3C_HB", -1);
    // at most FOUR (tile, block) slots per wave: the eight-slot instantiation needs more than the 512 registers (3 460 spilled,
    // and this compiler fails on its <8, false> form); a batch that needs more slots runs as several launches (pick_chunk)
    const int maxslots = std::min(4, std::max(1, env_int("PHX_V3C_SLOTS", 4)));
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
            if (fntg > 0 && fntg <= slots) { ntg = std::min(fntg, ntt); TG = (ntt + ntg - 1) / ntg; }
            else if (fntg == 0 && TPW == 1 && control != PHX_CTRL_SHARED) {
                // (one-tile groups may take three quarters of the chip -- 23 yeast pairs as two groups on 252 workgroups
                // measured +3 % --, two-tile groups all of it)
                for (int c = 1; c < ntg; c <<= 1) {
                    const int tgc = (ntt + c - 1) / c;
                    if ((long long)tgc * nblk * 2 * 4 <= (long long)cus * (c == 1 ? 3 : 4)) { ntg = c; TG = tgc; break; }
                }
            }
            const int Bt = 16 * ntg;
            const bool helpers = ntg < slots;
            if (control == PHX_CTRL_SHARED && TG != 1) continue;
            const size_t cb = ctl3c_bytes(Bt, ntg);
            for (int NB = 1; NB <= 8 && TPW * NB <= maxslots; NB <<= 1) {
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
                    best.nvec = NVEC_ADJ3C; best.BN = (long long)B * N; best.HC = HC; best.Hc = Hc;
                    best.Bcall = 0; best.cntN = (long long)B * N; best.res = res ? 1 : 0;
                    const int nslot = TPW * NB;
                    // half-block gene tiles (plan_fwd3c): one slot per wave and room for twice the workgroups
                    // (measured: -4..-37 % of a launch wherever twice the workgroups fit the chip)
                    const bool hb_fits = nslot == 1 && res && (long long)TG * G * 2 <= cus && cb + HSA_BYTES + 16 + blkbytes * HC <= LDS_BUDGET;
                    best.hb = (hb_fits && fhb != 0) ? 1 : 0;
                    // block split: a tile's gene blocks on the workgroup's spare waves (plan_fwd3c)
                    best.split = 1;
                    if (!best.hb && TPW == 1 && NB > 1 && ntg * NB <= NW && env_int("PHX_V3C_SPLIT", 1) != 0) {
                        const int parts = std::min(NW / ntg, NB);
                        if (hsa_offset(Bt, ntg) + spa_bytes(ntg, parts) + blkbytes * NB * (res ? HC : 1) <= LDS_BUDGET)
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

// floats of one batch group's partial: accumulator-native [gene block][chunk][4 HT x 2][64] float4, then dg [N], dbs [H], dbp [H]
size_t pp_adj3c(const D1 &d) { return align_up((size_t)d.nblk * d.HC * (4 * d.HT * 2 * 256) + d.N + 2 * d.H, 64); }

Regions make_layout3c(const D1 &d, bool grads)
{
    Regions L{};
    Take take;
    const size_t R = (size_t)d.ntg * d.HC * 4 * d.HT * 4 + d.ntg;   // hidden rows of every chunk + norm rows per group
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * R * 64 * 8);
    L.xbytes = take.off - L.part;                            // header + set 0: what a fill covers (phx_mfma_v3common.inc: XSet)
    L.part1 = take((size_t)d.TG * d.G * R * 64 * 8);         // set 1: cleaned by the launch that works in set 0
    L.zbuf1 = take((size_t)d.TG * R * 64 * 8);
    L.scratch = take((size_t)d.TG * d.G * NVEC_ADJ3C * d.ntg * d.NB * 512 * 4);
    L.pp = (long long)pp_adj3c(d);
    L.nparts = d.TG;   // one partial per batch group (the quadrature's items: every slot has one owner wave)
    // every item's owner first-touches its slots (plain stores) in the first quadrature visit, or zero-fills them at the
    // end of the launch when its group never stepped
    L.dtheta = take(grads ? pp_adj3c(d) * 4 * d.TG : 0);
    L.prof = take((size_t)d.TG * d.G * 16 * 8);
    L.wimg = take((size_t)d.nblk * d.HC * blk_floats_ch(d.HT, d.Hc) * 4);
    // transposed hidden rows of the seven ring slots, shared by a group's workgroups: [group][tile][7][chunk][4 HT][64] float4
    L.hq = take(grads ? (size_t)d.TG * d.ntg * 7 * d.HC * 4 * d.HT * 1024 : 0);
    L.total = take.off;
    return L;
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
    hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk * d.HC), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, d.HC, d.Hc,
                       blk_floats_ch(d.HT, d.Hc));
    a.lds = lds_bytes_adj3c(d);
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
                                    plan_adj3c, make_layout3c, plan6_chunked, prepare_adj3c, launch_adj3c, reduce_adj3c};
    return b;
}
}  // namespace phxh
