// phx_plan.hpp -- launch planning and workspace layout of the persistent solve kernels: host code only, shared by the
// kernel families' translation units and phx_engine.hip.  Every planner is a pure function of a Shape (the CU count is
// part of it: no planner asks the device) and of the diagnostic switches, which read_switches() takes from the live
// environment once per plan call, only those the family looks at.  Include after phx_host.hpp and phx_mfma_common.inc (blk_floats_ch, k1_pack_images).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {

using namespace phxh;

// The diagnostic switches of the planners (phoenix_amd/engine.py: _PLAN_ENV keys its caches with the same names).  A
// planner names the groups it looks at, so that a plan call -- several per solve call -- reads no switch it does not
// use; a field of a group that was not read holds the value of an unset variable.
enum SwitchGroup { SW_FWD = 1, SW_ADJ = 2, SW_MAXNW = 4, SW_V3_NB = 8, SW_ADJ2 = 16, SW_CHUNKED = 32 };
struct Switches {
    bool v0 = false;        // PHX_ENGINE=v0: no persistent MFMA kernel at all (always read)
    bool fwd_v1 = false;    // SW_FWD: PHX_FWD=v1 keeps every forward solve on k1_solve_fwd
    int adj = 0;            // SW_ADJ: PHX_ADJ=v1 / v2 / v3 forces that backward kernel: 1 / 2 / 3, else 0 (by shape)
    int v1_maxnw = 8;       // SW_MAXNW: PHX_V1_MAXNW, most waves per workgroup of k1_solve_fwd / adj / fwd3 (8: no cap)
    int v3_nb = 1;          // SW_V3_NB: PHX_V3_NB (experiment), smallest gene tile k1_solve_fwd3 / adj3 consider
    const char *adj2_np = nullptr;   // SW_ADJ2: PHX_ADJ2_NP, the wave pairs per workgroup of k1_solve_adj2 (0: both forms)
    // SW_CHUNKED, the hidden-chunked kernels:
    bool v3c_off = false;   // PHX_V3C=0 switches them off
    int v3c_nb = 0, v3c_tpw = 0;   // PHX_V3C_NB / PHX_V3C_TPW: the only NB / TPW they consider (0: all)
    int v3c_res = -1;       // PHX_V3C_RES=0: one re-staged chunk slot also where every chunk fits the LDS
    int v3c_hb = -1;        // PHX_V3C_HB: 0 = never half-block tiles, 1 = wherever they fit, else by the families' rules
    int v3c_ntg = 0;        // PHX_V3C_NTG: trajectory tiles per batch group (0: by rule; 4: the plan before that rule)
    bool v3c_split = true;  // PHX_V3C_SPLIT=0: no block split
    int v3c_slots = 4;      // PHX_V3C_SLOTS: (tile, block) slots per wave of k1_solve_adj3c, 1 .. 4
};

// from the live environment, once per plan call (never cached: tests and tools flip the switches between calls)
inline Switches read_switches(int groups)
{
    const auto num = [](const char *name, int dflt) {
        const char *e = getenv(name);
        return e ? atoi(e) : dflt;
    };
    Switches s;
    s.v0 = force_v0();
    if (groups & SW_FWD) {
        const char *f = getenv("PHX_FWD");
        s.fwd_v1 = f && strcmp(f, "v1") == 0;
    }
    if (groups & SW_ADJ) {
        const char *a = getenv("PHX_ADJ");
        s.adj = !a ? 0 : strcmp(a, "v1") == 0 ? 1 : strcmp(a, "v2") == 0 ? 2 : strcmp(a, "v3") == 0 ? 3 : 0;
    }
    if (groups & SW_MAXNW) s.v1_maxnw = std::max(1, num("PHX_V1_MAXNW", 8));
    if (groups & SW_V3_NB) s.v3_nb = std::max(1, num("PHX_V3_NB", 1));
    if (groups & SW_ADJ2) s.adj2_np = getenv("PHX_ADJ2_NP");
    if (groups & SW_CHUNKED) {
        const char *c = getenv("PHX_V3C");
        s.v3c_off = c && c[0] == '0';
        s.v3c_nb = num("PHX_V3C_NB", 0);
        s.v3c_tpw = num("PHX_V3C_TPW", 0);
        s.v3c_res = num("PHX_V3C_RES", -1);
        s.v3c_hb = num("PHX_V3C_HB", -1);
        s.v3c_ntg = num("PHX_V3C_NTG", 0);
        s.v3c_split = num("PHX_V3C_SPLIT", 1) != 0;
        s.v3c_slots = std::min(4, std::max(1, num("PHX_V3C_SLOTS", 4)));
    }
    return s;
}

// how a family cuts the hidden layer and what a gene block costs: HT tiles of 16 rows, HC chunks of Hc rows, private
// state vectors per workgroup, LDS bytes of one gene block's weight image (one chunk)
struct Tiles {
    int HT, HC, Hc, nvec;
    size_t blkbytes;
};
inline Tiles make_tiles(int HT, int HC, int Hc, int nvec) { return {HT, HC, Hc, nvec, (size_t)blk_floats_ch(HT, Hc) * 4}; }

// THE D1 constructor.  norms: the family has shared-control norm rows (D1::cntN) and takes several calls per launch
// (s.calls > 1: B = calls x Bcall rows, batch group g = call g); k1_solve_adj2 and k1_solve_bp leave both zero.
// res / hb / split are the chunked search's to set; K is the caller's (k1_solve_bp).
inline D1 make_d1(const Shape &s, const Tiles &t, int NW, int TPW, int NB, int TG, int ntg, bool norms = true)
{
    D1 d{};
    d.N = s.N; d.H = s.H; d.B = s.B; d.T = s.T; d.HT = t.HT; d.NB = NB; d.NW = NW; d.TPW = TPW;
    d.nblk = (s.N + 31) / 32; d.G = (d.nblk + NB - 1) / NB; d.TG = TG; d.ntg = ntg; d.Bt = 16 * ntg;
    d.nvec = t.nvec; d.BN = (long long)s.B * s.N; d.HC = t.HC; d.Hc = t.Hc;
    if (norms) {
        d.Bcall = s.calls > 1 ? s.B / s.calls : 0;
        d.cntN = (long long)(d.Bcall ? d.Bcall : s.B) * s.N;
    }
    return d;
}

// The search of the families that keep a gene tile's weights LDS resident (k1_solve_fwd / adj, fwd3, adj3): (NW, TPW)
// from `nwmax` waves down, TPW in {1, 2, 4}, and per pair the smallest NB from `nb_first` on whose TG x G workgroups the
// `cus` hold -- the cheapest of the pair.  Cost: the per-SIMD MFMA work TPW * NB * ceil(NW / 4) first; then, where the
// family prefers full workgroups (full_nw > 0: the forward kernels are light on registers and measured faster with
// more waves), 100 per halving below full_nw; then the smallest batch group (exchange volume, members per reduction);
// a single group smaller than its wave slots is preferred, its spare waves help the exchange.
// ctl(NW, TPW, TG, ntg, Bt): the LDS bytes beside the weight images.
// s.calls > 1 (shared control only): one batch group per call, so a call must fit one group.
template <typename Ctl>
bool plan_resident(const Shape &s, const Tiles &t, int nwmax, int full_nw, int nb_first, Ctl ctl, D1 *out)
{
    if (s.cus <= 0 || (s.calls > 1 && (s.control != PHX_CTRL_SHARED || s.B % s.calls != 0))) return false;
    const int Bcall = s.calls > 1 ? s.B / s.calls : 0;
    const int nblk = (s.N + 31) / 32, ntt = ((Bcall ? Bcall : s.B) + 15) / 16;
    long long best_cost = -1;
    for (int NW = nwmax; NW >= 1; NW >>= 1)
        for (int TPW = 1; TPW <= 4; TPW <<= 1) {
            const int slots = NW * TPW, TG = Bcall ? s.calls : (ntt + slots - 1) / slots;
            if (Bcall && slots < ntt) continue;   // a call is one group
            const int ntg = (TG == 1 || Bcall) ? std::min(slots, ntt) : slots, Bt = 16 * ntg;
            const bool helpers = ntg < slots;
            if (s.control == PHX_CTRL_SHARED && TG != 1 && !Bcall) continue;
            const size_t cb = ctl(NW, TPW, TG, ntg, Bt);
            if (cb + t.blkbytes > LDS_BUDGET) continue;
            const int NBmax = (int)std::min<size_t>((LDS_BUDGET - cb) / t.blkbytes, 8);
            for (int NB = nb_first; NB <= NBmax; ++NB) {
                if ((long long)TG * ((nblk + NB - 1) / NB) > s.cus) continue;
                const long long cost = (long long)TPW * NB * ((NW + 3) / 4) * 1000 + (full_nw ? (full_nw - NW) * 100 : 0) +
                                       Bt / 4 - (helpers && TPW == 1 ? 50 : 0);
                if (best_cost < 0 || cost < best_cost) {
                    best_cost = cost;
                    *out = make_d1(s, t, NW, TPW, NB, TG, ntg);
                }
                break;  // smallest feasible NB for this (NW, TPW) is the cheapest
            }
        }
    return best_cost >= 0;
}

// the shapes of the hidden-chunked families (asked before the switches are read: most shapes are turned away here)
inline bool chunked_shape(const Shape &s) { return s.cus > 0 && s.method == PHX_DOPRI5 && s.H > 48 && s.H <= 256; }

// What differs between the two hidden-chunked kernels (k1_solve_fwd3c / adj3c) in the search below.
struct ChunkedRules {
    int nvec;
    int maxslots;      // (tile, block) slots per wave the kernel is built for
    int wide_share;    // quarters of the chip that groups of two or more tiles may take with half-block tiles
    bool forward;      // k1_solve_fwd3c: takes several calls (plan_resident's rule), its controllers step one trajectory
                       // per thread (Bt <= 64 * NW), and half-block tiles only pay for small groups
    size_t hb_bytes;   // LDS of the half-block combine
};

// The search of the hidden-chunked families, 48 < H <= 256: HC = ceil(H / 48) chunks of Hc = ceil(H / HC) rows, three
// 16-row tiles each (120 -> 3 x 40, 200 -> 5 x 40).  (NW, TPW, NB): one wave per SIMD, gene tiles of 1 / 2 / 4 / 8 blocks,
// at most maxslots (tile, block) slots per wave (the kernels keep their partial sums in registers); all chunks LDS
// resident when they fit, else one re-staged slot.  Cost: the per-wave MFMA work first, then the exchange volume
// (members per group).  ctl(Bt, ntg): control LDS; split_lds(Bt, ntg, parts): control LDS of the block-split form.
template <typename Ctl, typename SplitLds>
bool plan_chunked(const Shape &s, const Switches &sw, const ChunkedRules &r, Ctl ctl, SplitLds split_lds, D1 *out)
{
    if (!chunked_shape(s) || (s.calls > 1 && (!r.forward || s.control != PHX_CTRL_SHARED || s.B % s.calls != 0))) return false;
    const int Bcall = s.calls > 1 ? s.B / s.calls : 0;
    const int HC = (s.H + 47) / 48;
    const Tiles t = make_tiles(3, HC, (s.H + HC - 1) / HC, r.nvec);
    const int nblk = (s.N + 31) / 32, ntt = ((Bcall ? Bcall : s.B) + 15) / 16;
    long long best_cost = -1;
    for (int NW = 4; NW >= 1; NW >>= 1)
        for (int TPW = 1; TPW <= 8; TPW <<= 1) {
            if (sw.v3c_tpw > 0 && TPW != sw.v3c_tpw) continue;
            const int slots = NW * TPW;
            int TG = (ntt + slots - 1) / slots;
            int ntg = TG == 1 ? std::min(slots, ntt) : slots;
            // More batch groups of FEWER trajectory tiles where the chip has room for them (one tile per wave plans, twice
            // the gene blocks -- half-block tiles -- still resident): the groups' exchanges carry fewer rows and a tile gets
            // helper waves (measured: -8 ... -32 % of a launch; 23 yeast pairs as two groups of one tile: neutral).
            if (Bcall) {   // a call is one group
                if (slots < ntt) continue;
                TG = s.calls; ntg = ntt;
            } else if (sw.v3c_ntg > 0 && sw.v3c_ntg <= slots) { ntg = std::min(sw.v3c_ntg, ntt); TG = (ntt + ntg - 1) / ntg; }
            else if (sw.v3c_ntg == 0 && TPW == 1 && s.control != PHX_CTRL_SHARED) {
                // one-tile groups may take three quarters of the chip (backward: 23 yeast pairs as two groups on 252
                // workgroups measured +3 %), groups of more tiles wide_share quarters: half of it forward (beyond, the
                // launch measured +8 ... +18 % -- 252 half-block workgroups at two tiles per group), all of it backward
                for (int c = 1; c < ntg; c <<= 1) {
                    const int tgc = (ntt + c - 1) / c;
                    if ((long long)tgc * nblk * 2 * 4 <= (long long)s.cus * (c == 1 ? 3 : r.wide_share)) { ntg = c; TG = tgc; break; }
                }
            }
            const int Bt = 16 * ntg;
            // forward: a group of more trajectories than the workgroup has threads (eight-tile waves, more than 16 tiles)
            // would leave the rest unsolved
            if (r.forward && Bt > 64 * NW) continue;
            const bool helpers = ntg < slots;
            if (s.control == PHX_CTRL_SHARED && TG != 1 && !Bcall) continue;
            const size_t cb = ctl(Bt, ntg);
            for (int NB = 1; NB <= 8 && TPW * NB <= r.maxslots; NB <<= 1) {
                if (sw.v3c_nb > 0 && NB != sw.v3c_nb) continue;
                if (cb + t.blkbytes * NB > LDS_BUDGET) break;
                const int G = (nblk + NB - 1) / NB;
                if ((long long)TG * G > s.cus) continue;
                const bool res = sw.v3c_res != 0 && cb + t.blkbytes * NB * HC <= LDS_BUDGET;
                const long long cost = (long long)TPW * NB * 1000 + (res ? 0 : 150) + G - (helpers && TPW == 1 ? 50 : 0);
                if (best_cost >= 0 && cost >= best_cost) continue;
                best_cost = cost;
                D1 &d = *out;
                d = make_d1(s, t, NW, TPW, NB, TG, ntg);
                d.res = res ? 1 : 0;
                // HALF-BLOCK gene tiles: a plan of one slot per wave with room for twice the workgroups (twice the
                // workgroups, half the sweep work each; backward: -4..-37 % of a launch wherever they fit).  Forward
                // (H = 120 / 200, 8..220 gene blocks, 16..128 trajectories): -9..-33 % while the groups' rows times their
                // workgroups stay small (four-tile groups on at most half the chip, one-tile groups on all of it) and a
                // group has at most 160 members; +5..+24 % beyond (tools/v3c_check.py hbgrid)
                const bool hb_fits = TPW * NB == 1 && res && (long long)TG * G * 2 <= s.cus &&
                                     cb + r.hb_bytes + 16 + t.blkbytes * HC <= LDS_BUDGET;
                d.hb = (hb_fits && sw.v3c_hb != 0 &&
                        (!r.forward || sw.v3c_hb == 1 || ((long long)TG * G * ntg <= s.cus && 2 * nblk <= 160))) ? 1 : 0;
                // block split: a tile's gene blocks on the workgroup's spare waves (small batches of multi-block tiles)
                d.split = 1;
                if (!d.hb && TPW == 1 && NB > 1 && ntg * NB <= NW && sw.v3c_split) {
                    const int parts = std::min(NW / ntg, NB);
                    if (split_lds(Bt, ntg, parts) + t.blkbytes * NB * (res ? HC : 1) <= LDS_BUDGET) d.split = parts;
                }
            }
        }
    if (best_cost < 0) return false;
    if (out->hb) out->G = 2 * out->nblk;
    return true;
}

// What a family's workspace layout adds to the regions all of them share.
struct LayoutSpec {
    size_t part_rows, zbuf_rows;   // exchange rows (64 granules each) per workgroup / per batch group
    int zslots = 1;                // reduced-row slots of the one exchange set
    bool two_sets = false;         // third generation: a second exchange set, cleaned by the launch that works in set 0
    bool prof = true;              // per-workgroup segment timers
    // tail / has_hq say whether the family TAKES the region, also with zero bytes (no gradients wanted): a taken region
    // reports the offset it would start at, one never taken reports 0 -- the offsets the kernels have always been given
    bool tail = false;             // backward (and k1_solve_fwd, which shares k1_solve_adj's layout): gradient partials
    long long pp = 0;              //   floats per partial
    int nparts = 0;                //   partials the gradient reduce sums
    size_t dtheta = 0;             //   bytes of all partials
    bool has_hq = false;           // transposed hidden rows of the quadrature
    size_t hq = 0;
};

// THE layout builder: regions 256-byte aligned, in this order; a region a family does not have keeps offset 0
inline Regions make_regions(const D1 &d, const LayoutSpec &s)
{
    Regions L{};
    Take take;
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * s.part_rows * 64 * 8);
    L.zbuf = take((size_t)s.zslots * d.TG * s.zbuf_rows * 64 * 8);
    L.xbytes = take.off - L.part;   // header + set 0: what a fill covers
    if (s.two_sets) {
        L.part1 = take((size_t)d.TG * d.G * s.part_rows * 64 * 8);
        L.zbuf1 = take((size_t)d.TG * s.zbuf_rows * 64 * 8);
    }
    L.scratch = take((size_t)d.TG * d.G * d.nvec * d.ntg * d.NB * 512 * 4);
    if (s.tail) {
        L.pp = s.pp;
        L.nparts = s.nparts;
        L.dtheta = take(s.dtheta);
    }
    L.prof = take(s.prof ? (size_t)d.TG * d.G * 16 * 8 : 0);
    L.wimg = take((size_t)d.nblk * d.HC * blk_floats_ch(d.HT, d.Hc) * 4);
    if (s.has_hq) L.hq = take(s.hq);
    L.total = take.off;
    return L;
}

// The weight images a launch reads: the caller's (phx_params.wimg, packed once for these parameter values) where the
// family reads that format, else packed into the workspace in front of the launch.
inline void pack_images(SolveArgs &a, const phx_params *p, hipStream_t st, bool callers_format = true)
{
    const D1 &d = a.d;
    if (callers_format && p->wimg) a.w.wimg = (const float *)p->wimg;
    else
        hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk * d.HC), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, d.HC,
                           d.Hc, blk_floats_ch(d.HT, d.Hc));
}

}  // namespace
