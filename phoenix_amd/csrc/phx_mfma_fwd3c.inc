// phx_mfma_fwd3c.inc -- third-generation forward solve for WIDE hidden layers (H > 48: the yeast shape C3, H = 120, and the
// B-cell shape C5, H = 200): odeint(ODENet, y0, t) for dopri5.  Same algorithm, layouts, exchange protocol, controller
// arithmetic and private-state byte stream as k1_solve_fwd3 (phx_mfma_fwd3.inc; reference: odeint.py, rk_common.py:39-228,
// misc.py:47-103, interp.py, odenet.py:85-91): 8 private vectors, fused sweeps, ring FSAL, granule pairs, two exchange sets.
// What is new is the HIDDEN-CHUNK dimension:
//   * the hidden layer is cut into HC chunks of Hc <= 48 rows (H = 120: 3 x 40, H = 200: 5 x 40), each chunk a three-tile
//     slice exactly like the narrow kernel's whole layer (HALF: a chunk of <= 40 rows skips the padding k-steps / pairs);
//     f = relu(g) (sum_c W_alpha[:, c] z_c - y): every product is a sum over chunks or produces per-chunk rows;
//   * a sweep is THREE phases: (A) the expansion partial sums j += W_alpha[:, c] z_c of chunks 0 .. HC-2 into per-(tile,
//     block) accumulators that stay in registers; (F) the fused visit of the narrow kernel with the LAST chunk (finishes
//     j, forms k_s, the next stage input and its activations, contracts them with the last chunk's Ws / Wp rows);
//     (C) the contractions of chunks HC-2 .. 0 from the activations kept in registers.  The tile stream (loads / stores of
//     the private vectors) is the narrow kernel's: once per block visit, under the MFMAs of phase F;
//   * LDS holds either the images of ALL chunks of the workgroup's gene blocks (`d.res`: yeast, 3 x 22 KB per block) or ONE
//     chunk slot that the phases re-stage as they walk the chunks (B-cell: 230 KB of images per four-block gene tile);
//     phase C walks the chunks backwards so that a sweep starts with the chunk its predecessor left resident
//     (2 HC - 2 stagings per sweep);
//   * the (tile, block) loops of a wave are fully unrolled over NBT slots (accumulators / activations indexed at compile
//     time); gene tiles are 1, 2, 4 or 8 blocks.
namespace {

enum { FC_Y0 = 0, FC_K = 1 };
constexpr int NVEC_FWD3C = 8;

__host__ __device__ inline size_t ctlf3c_bytes(int Bt, int ntg) { return ctl_bytes(Bt) + (size_t)ntg * 8 + 64; }
// half-block tiles whose workgroup has spare waves: the hand-over region behind the controllers (partial sums of the
// helpers [4 waves][64] f32x4, then the owners' activations [2 tiles][8][64] floats)
constexpr size_t HSF_BYTES = 4096 + 4096;
__host__ __device__ inline size_t hsf_offset(int Bt, int ntg) { return (ctlf3c_bytes(Bt, ntg) + 15) & ~(size_t)15; }
// block split (d.split > 1: small batches of multi-block gene tiles): the partial rows of the waves beyond a tile's first,
// [(part - 1) ntg + tile][2 HT accumulators + one norm row][64] in the same place
__host__ __device__ inline size_t spf_bytes(int ntg, int parts) { return (size_t)(parts - 1) * ntg * (2 * 3 * 1024 + 256); }

// CALLS: as in k1_solve_fwd3 -- d.TG independent shared-control calls of d.Bcall rows, one batch group and one time row each
// CLAMP (only with CALLS): as in k1_solve_fwd3 -- call g reads relu(g) of its clamp_width genes of clamp_gene as 0 in
// every sweep
template <int NBT, bool HALF, bool HB, bool CALLS = false, bool CLAMP = false>
__global__ __launch_bounds__(256) void k1_solve_fwd3c(Net net, D1 d, W1 w, SolveCfg cfg, const float *__restrict__ y0,
                                                      const double *__restrict__ t, float *sol, int *status,
                                                      int *nfe_out, int *nsteps_out, const int *__restrict__ clamp_gene,
                                                      int clamp_width)
{
    static_assert(!CLAMP || CALLS, "a clamped gene belongs to a call");
    constexpr int HT = 3, F2 = 2 * HT;
    // HB: HALF-BLOCK gene tiles (small batches of a single-slot plan): the workgroup owns the 16 genes of half `s2w` of block
    // gt >> 1 -- its sweeps cost half the MFMAs and vector work of a one-block tile, the price is twice the exchange members
    constexpr int GW = HB ? 4 : 8;       // genes per lane in the workgroup's part of a tile slot
    static_assert(!HB || NBT == 1, "half-block tiles: one (tile, block) slot per wave");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tile / row offsets stay scalar
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int s2w = HB ? (gt & 1) : 0, goff = 4 * s2w;
    const int blk0 = HB ? (gt >> 1) : gt * d.NB;
    const int nbl = HB ? 1 : min(d.NB, d.nblk - blk0);
    const int lnb = __builtin_ctz((unsigned int)d.NB);   // gene tiles are 1, 2, 4 or 8 blocks
    const int N = d.N, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G, HC = d.HC;
    const int BLKF = blk_floats_ch(HT, d.Hc);
    const bool shared = cfg.control == PHX_CTRL_SHARED;
    auto rowof = [&](int lb) -> int { return CALLS ? (lb < d.Bcall ? grp * d.Bcall + lb : B) : grp * Bt + lb; };
    const int trow_sh = CALLS ? grp : 0;
    ClampSet cset{};   // the call's held genes
    if constexpr (CLAMP) cset = clamp_set(clamp_gene, grp, clamp_width);
    auto pair_live = [](int k) -> bool { return !(HALF && (k >> 1) % HT == HT - 1 && (k & 1)); };
    auto hc_of = [&](int c) -> int { return min(d.Hc, d.H - c * d.Hc); };
    const int cstride = d.res ? d.NB * BLKF : 0;   // floats between the chunk slots of the LDS images (0: one slot)
    float *ctlbase = lds + (long long)(d.res ? HC : 1) * d.NB * BLKF;
    Ctl c = carve_ctl(ctlbase, Bt);
    int *kbs = reinterpret_cast<int *>(reinterpret_cast<char *>(ctlbase) + ctl_bytes(Bt));   // [ntg] ring base of the tile
    int *rotf = kbs + ntg;                                                                      // [ntg] ring turns now
    float *hsP = reinterpret_cast<float *>(reinterpret_cast<char *>(ctlbase) + hsf_offset(Bt, ntg));   // (HB only)
    float *hsA = hsP + 1024;
    const int NPT = HC * F2 * 2;     // row pairs of one trajectory tile: [chunk][section tile][half]
    const int RH = ntg * NPT * 2;    // hidden rows (u, v of every chunk) of one exchange; norm rows follow
    const int R = RH + ntg;
    unsigned long long *xpart, *xzbuf;
    unsigned int *xabort;
    const XSet xs = xset_begin(w, grp, gt, G, R, xpart, xzbuf, xabort);
    Xchg x{xpart, xzbuf, 0, xabort, 0u, G, gt, R, false};
    const __amdgpu_buffer_rsrc_t prs = make_rsrc(x.part, (unsigned int)((size_t)G * R * 512));
    const __amdgpu_buffer_rsrc_t zrs = make_rsrc(x.zbuf, (unsigned int)((size_t)R * 512));
    const int lane16x = lane * 16;
    auto st_pair = [&](__amdgpu_buffer_rsrc_t rs, int byte_off, float v0, float v1, unsigned int tag) {
        const i32x4 u = {__float_as_int(v0), (int)tag, __float_as_int(v1), (int)tag};
        store128<16>(u, rs, lane16x, byte_off);   // + the store-data hazard guard (phx_mfma_v3common.inc)
    };
    auto ld_pair = [&](__amdgpu_buffer_rsrc_t rs, int byte_off) -> i32x4 {
        return __builtin_amdgcn_raw_buffer_load_b128(rs, lane16x, byte_off, (int)0x80000010);   // sc1, volatile
    };
    SegTimer tm;
    tm.start(w.prof != nullptr, c.tacc);

    // ---- weights: every chunk (resident form) or the chunk the first sweep starts with (the last one)
    int cur = HC - 1;   // the chunk in the slot (one-slot form); workgroup uniform
    if (d.res) {
        for (int ch = 0; ch < HC; ++ch) stage_chunk_flat<8>(w.wimg, lds + (long long)ch * cstride, blk0, nbl, ch, HC, BLKF);
    } else {
        stage_chunk_flat<24>(w.wimg, lds, blk0, nbl, cur, HC, BLKF);
    }
    const int offR = rho16(li >> 2, li & 3) * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = rho16(lq, 0) * LROW + gmapC(li, 0);
    offC[1] = rho16(lq, 0) * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * d.nvec * tiles_wg * 512;
    const __amdgpu_buffer_rsrc_t trs = make_rsrc(wgbase, (unsigned int)(d.nvec * tiles_wg * 2048));
    auto toff = [&](int v, int ttl, int bl) -> int { return ((v * tiles_wg) + (ttl * d.NB + bl)) * 2048; };
    auto ring = [&](int kb, int j) -> int { const int v = kb + j; return v >= 7 ? v - 7 : v; };

    // ---- controllers (replicated in every workgroup of the group; deterministic => identical)
    for (int lb = tid; lb < Bt; lb += blockDim.x) {
        const int b = rowof(lb);
        const bool vb = b < B;
        const TimeRow tb = trowT(t, T, cfg, shared ? trow_sh : (vb ? b : 0));
        float sg = 1.0f;
        int st = PHX_OK;
        if (T >= 2) {
            sg = (tb[1] < tb[0]) ? -1.0f : 1.0f;
            for (int i = 0; i + 1 < T; ++i)
                if (!((double)sg * tb[i + 1] > (double)sg * tb[i])) st = PHX_ERR_BAD_ARG;
        }
        c.sgn[lb] = sg; c.st[lb] = st; c.nsteps[lb] = 0; c.nfe[lb] = 0; c.nsiv[lb] = 0;
        c.rk_t0[lb] = (double)sg * tb[0]; c.rk_t1[lb] = (double)sg * tb[0];
        c.out_idx[lb] = 1;
        c.done[lb] = (!vb || T < 2 || st != PHX_OK) ? 1 : 0;
        c.accept[lb] = 0; c.fin[lb] = 0; c.out_lo[lb] = 1; c.out_hi[lb] = 1;
        c.dtf[lb] = 0.f; c.h0f[lb] = 0.f; c.dtp[lb] = 0.f; c.d1[lb] = 0.f; c.dt[lb] = 0.0;
    }
    for (int i = tid; i < ntg; i += blockDim.x) { kbs[i] = 0; rotf[i] = 0; }
    // ---- initial state: Y0 tiles <- y0, sol[0] <- y0
    for (int s = 0; s < d.TPW; ++s) {
        const int ttl = wv * d.TPW + s;
        if (ttl >= ntg) continue;
        const int b = rowof(ttl * 16 + li);
        for (int bl = 0; bl < nbl; ++bl) {
            float xv[GW];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, goff);
            row_loadG<GW>(y0, (long long)b * N, g0, N, b < B, 0.5f, xv);
            row_storeG<GW>(sol, (long long)b * N, g0, N, b < B, xv);
#pragma unroll
            for (int j = 0; j < GW; ++j)
                if (g0 + j >= N) xv[j] = 0.5f;   // padding genes: a = l = 0
            tstore<GW>(trs, lane * 32 + 4 * goff, toff(FC_Y0, ttl, bl), xv);
        }
    }
    __syncthreads();
    tm.mark(6);

    auto count_active = [&]() -> int {   // trajectories of the group that still integrate (every thread gets the count)
        __syncthreads();
        const unsigned long long mine = __ballot(tid < Bt && !c.done[tid]);
        if (lane == 0) c.misc[4 + wv] = __popcll(mine);
        __syncthreads();
        int n = 0;
        for (int k = 0; k < d.NW; ++k) n += c.misc[4 + k];
        return n;
    };

    // members' pairs [first + k step] of pair row `pr` until both halves of every one carry the tag
    auto poll_pairs = [&](int pr, int first, int step, int nv, float &s0, float &s1) {
        constexpr int NL = 16;
        i32x4 g[NL];
        unsigned int spins = 0;
        unsigned long long t_start = 0;
        for (;;) {
#pragma unroll
            for (int k = 0; k < NL; ++k) g[k] = ld_pair(prs, (min(first + k * step, G - 1) * R * 64 + pr * 128) * 8);
            bool ok = true;
#pragma unroll
            for (int k = 0; k < NL; ++k) ok = ok && (k >= nv || ((unsigned int)g[k].y == x.tag && (unsigned int)g[k].w == x.tag));
            if (__all(ok) || x.aborted) break;
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 255u) == 0) {
                if (t_start == 0) t_start = wall_clock64();
                if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                    wall_clock64() - t_start > 500000000ull) {
                    __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    x.aborted = true;
                }
            }
        }
        s0 = 0.f; s1 = 0.f;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            s0 += (k < nv) ? __int_as_float(g[k].x) : 0.f;
            s1 += (k < nv) ? __int_as_float(g[k].z) : 0.f;
        }
    };
    // hidden exchange: reduce-scatter of the partial row pairs of the current exchange (tag x.tag), pair ownership p mod G
    auto reduce_hidden = [&]() {
        tm.mark(0);
        auto post = [&](int u, float tot) -> float {   // row u of the group: ((tile HC + chunk) F2 + f2) 4 + r
            const int r = u & 3, q4 = u >> 2, f2 = q4 % F2, ch = (q4 / F2) % HC;
            const int rc = 16 * (f2 % HT) + rho16(lq, r);
            if (rc >= hc_of(ch)) return 0.f;
            const int row = ch * d.Hc + rc;
            return (f2 < HT) ? tot + net.bs[row] : expf(tot + net.bp[row]);
        };
        // ownership over the LIVE pairs only (HALF: every sixth pair holds padding rows), so that the members' shares differ by
        // at most one pair -- the slowest member's share is the exchange's latency
        constexpr int U = F2 * 2, LU = HALF ? U - U / 6 : U;
        const int NL = (RH / 2 / U) * LU;
        auto live_pair = [&](int dl) -> int { const int un = dl / LU, r = dl - un * LU; return un * U + (HALF ? r + r / 5 : r); };
        // Two forms: every wave reduces pairs of its own (the members in polls of 16; no barrier), or the four waves split the
        // members of one pair (sums combined through LDS).  The form with fewer polls in a row on the slowest member wins.
        const int cnt = (NL + G - 1) / G;
        // (measured, round 5: 19..32 members -30..-40 % of a launch against the split form; 230 members, 15 polls against 16: +3 %)
        const bool per_wave = G <= 128 && ((cnt + d.NW - 1) / d.NW) * ((G + 15) / 16) <= cnt * ((G + 16 * d.NW - 1) / (16 * d.NW));
        if (per_wave) {
            for (int dl = gt + wv * G; dl < NL; dl += G * d.NW) {
                const int p = live_pair(dl);
                float s0 = 0.f, s1 = 0.f;
                for (int g0 = 0; g0 < G; g0 += 16) {
                    float a0, a1;
                    poll_pairs(p, g0, 1, min(16, G - g0), a0, a1);
                    s0 += a0; s1 += a1;
                }
                st_pair(zrs, p * 1024, post(2 * p, s0), post(2 * p + 1, s1), x.tag);
            }
        } else {
            for (int dl = gt; dl < NL; dl += G) {
                const int p = live_pair(dl);
                float s0 = 0.f, s1 = 0.f;
                for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                    int nv = 0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) nv += (g2 + k * d.NW < G) ? 1 : 0;
                    float a0, a1;
                    poll_pairs(p, g2, d.NW, nv, a0, a1);
                    s0 += a0; s1 += a1;
                }
                // combine through LDS ([row of the pair][wave]): wave 0 publishes
                c.wred[(0 * 8 + wv) * 64 + lane] = s0;
                c.wred[(1 * 8 + wv) * 64 + lane] = s1;
                __syncthreads();
                if (wv == 0) {
                    float t0 = c.wred[lane], t1 = c.wred[8 * 64 + lane];
                    for (int k = 1; k < d.NW; ++k) { t0 += c.wred[k * 64 + lane]; t1 += c.wred[(8 + k) * 64 + lane]; }
                    st_pair(zrs, p * 1024, post(2 * p, t0), post(2 * p + 1, t1), x.tag);
                }
                __syncthreads();   // the combine buffer is reused by the next pair / the norm reduction
            }
        }
        tm.mark(3);
    };
    // norm rows (8-byte granules): reduce-scatter by row ownership, then every controller's value through LDS
    auto reduce_norm_rows = [&]() {
        for (int u = gt; u < ntg; u += G) {
            const int row = RH + u;
            float sacc = 0.f;
            for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                const u64 *rows[16];
                int nv = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int gg = g2 + k * d.NW;
                    rows[k] = x.part + ((long long)min(gg, G - 1) * R + row) * 64;
                    nv += (gg < G) ? 1 : 0;
                }
                float v[16];
                wait_rows<16>(x, rows, nv, lane, v);
#pragma unroll
                for (int k = 0; k < 16; ++k) sacc += (k < nv) ? v[k] : 0.f;
            }
            c.wred[wv * 64 + lane] = sacc;
            __syncthreads();
            if (wv == 0) {
                float tot = c.wred[lane];
                for (int k = 1; k < d.NW; ++k) tot += c.wred[k * 64 + lane];
                st_gran(x.zbuf + (long long)row * 64, lane, tot, x.tag);
            }
            __syncthreads();
        }
    };
    auto norms = [&](int nslots, float *out /* per-thread result [nslots] */) {
        reduce_norm_rows();
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;
            const u64 *rows[1] = {x.zbuf + (long long)(RH + ttl) * 64};
            float v[1];
            wait_rows<1>(x, rows, 1, lane, v);
            c.nrm[ttl * 64 + lane] = v[0];
        }
        __syncthreads();
        double v2[2] = {0.0, 0.0};
        if (tid < Bt && rowof(tid) < B)
            for (int k = 0; k < nslots; ++k) v2[k] = (double)c.nrm[(tid >> 4) * 64 + k * 16 + (tid & 15)];
        if (!shared) {
            for (int k = 0; k < nslots; ++k) out[k] = sqrtf((float)(v2[k] / (double)N));
            __syncthreads();
            tm.mark(8);
            return;
        }
        if (tid < Bt)
            for (int k = 0; k < nslots; ++k) c.tmpd[k * Bt + tid] = v2[k];
        __syncthreads();
        for (int k = 0; k < nslots; ++k) {
            double sacc = 0.0;
            for (int lb = 0; lb < Bt; ++lb) sacc += c.tmpd[k * Bt + lb];
            out[k] = sqrtf((float)(sacc / (double)d.cntN));
        }
        __syncthreads();
        tm.mark(8);
    };

    // -----------------------------------------------------------------------------------------------------------
    // One sweep over this wave's tiles (see the file header and k1_solve_fwd3).  NK k tiles read; DO2: finish stage NK
    // (gather its hidden rows of exchange tagIn, recompute its input, P2 over all chunks, k_NK; RM 1: store k, norms
    // d0 / d1; 2: no store, norm d2; 3: store k, error ratio; 0: store k); DO1: form the next stage input, activations, P1
    // of every chunk into exchange tagOut.  cmode 1: the single coefficient is h0, 2: dopri5 tableau rows.
    // -----------------------------------------------------------------------------------------------------------
    auto sweep = [&](auto NKc, auto D2c, auto D1c, auto RMc, int cmode, unsigned int tagIn, unsigned int tagOut,
                     unsigned int tagN) {
        constexpr int NK = decltype(NKc)::value;
        constexpr bool DO2 = decltype(D2c)::value != 0, DO1 = decltype(D1c)::value != 0;
        constexpr int RM = decltype(RMc)::value;
        constexpr bool STK = DO2 && RM != 2;
        constexpr bool SK1 = DO2 && !DO1 && NK == 6;   // last stage: beta_72 = c_err2 = 0, k_2 is not read
        constexpr int NKL = NK > 0 ? NK : 1;
        tm.mark(0);
        // opaque copies: keeps the derived LDS / tile addresses of every sweep variant from being hoisted to the kernel top
        int BLKF_ = __builtin_amdgcn_readfirstlane(BLKF), cstr = __builtin_amdgcn_readfirstlane(cstride), offR_ = offR, offC0 = offC[0], offC1 = offC[1], lane32 = lane * 32 + 4 * goff;
        asm volatile("" : "+s"(BLKF_), "+s"(cstr));
        asm volatile("" : "+v"(offR_), "+v"(offC0), "+v"(offC1), "+v"(lane32));
        const int RGOFF = BLKF_ - 32;
        // One-slot form: the NEXT chunk is requested while the current one computes (chunk_issue: the loads fly under the MFMA
        // phases, the values wait in registers) and written to the slot between the two barriers of the switch.
        constexpr int PFN = 24;   // (declared inside the sweep: at kernel scope, behind two closure levels, the array is not promoted to registers)
        const bool pf_on = !d.res && d.NB <= 4;      // 24 float4 per thread hold a chunk of up to four gene blocks
        v4f pf[PFN];
        int pf_ch = -1;
        auto prefetch = [&](int ch) {
            if (pf_on && ch != cur) { chunk_issue<PFN>(w.wimg, blk0, nbl, ch, HC, BLKF, pf); pf_ch = ch; }
        };
        auto ensure_chunk = [&](int ch, int slot) {   // every wave of the workgroup calls this with the same sequence of chunks
            if (!d.res && cur != ch) {
                tm.mark(slot);                           // (the phase's compute up to here)
                __syncthreads();                         // every wave is done with the chunk in the slot
                tm.mark(13);                             // (waiting for the slowest wave)
                if (pf_ch == ch) chunk_commit<PFN>(lds, nbl, BLKF, pf);
                else stage_chunk_flat<24>(w.wimg, lds, blk0, nbl, ch, HC, BLKF);
                pf_ch = -1;
                __syncthreads();
                cur = ch;
                tm.mark(7);
            }
        };
        f32x4 pj[NBT][2];        // phase A: expansion partial sums of chunks 0 .. HC-2 per (tile, block) slot
        float avq[NBT][2 * GW];  // activations a | l of the next stage input per slot (phase C's B operands)
        float zr[F2][4];         // gathered hidden rows of one (tile, chunk)
        // gather the reduced rows of chunk `ch` of tile `ttl` (exchange `tag`): F2 x 2 pairs in one round trip
        auto gather = [&](int ttl, int ch, unsigned int tag) {
            constexpr int NPC = F2 * 2;
            const int pb = (ttl * NPT + ch * NPC) * 1024;
            i32x4 g[NPC];
#pragma unroll
            for (int k = 0; k < NPC; ++k) g[k] = pair_live(k) ? ld_pair(zrs, pb + k * 1024) : (i32x4){0, 0, 0, 0};
            unsigned int spins = 0;
            unsigned long long t_start = 0;
            for (;;) {
                bool ok = true;
#pragma unroll
                for (int k = 0; k < NPC; ++k)
                    ok = ok && (!pair_live(k) || ((unsigned int)g[k].y == tag && (unsigned int)g[k].w == tag));
                if (__all(ok) || x.aborted) break;
                __builtin_amdgcn_s_sleep(2);
#pragma unroll
                for (int k = 0; k < NPC; ++k)
                    if (pair_live(k)) g[k] = ld_pair(zrs, pb + k * 1024);
                if ((++spins & 255u) == 0) {
                    if (t_start == 0) t_start = wall_clock64();
                    if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                        wall_clock64() - t_start > 500000000ull) {
                        __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        x.aborted = true;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NPC; ++k) {   // pair k = (f2, r >> 1): rows r = 2 (k & 1), + 1
                zr[k >> 1][2 * (k & 1)] = __int_as_float(g[k].x);
                zr[k >> 1][2 * (k & 1) + 1] = __int_as_float(g[k].z);
            }
        };
        // j += W_alpha[:, chunk] z_chunk for one gene block (the two gene halves are independent chains, issued alternately)
        auto p2 = [&](const float *Wb, int hcc, f32x4 &aj0, f32x4 &aj1) {
            const float *Wc0 = Wb + (HB && s2w ? offC1 : offC0), *Wc1 = Wb + offC1;   // (HB: ONE chain, the workgroup's gene half)
#pragma unroll
            for (int f2 = 0; f2 < F2; ++f2) {
                const int rb = (f2 < HT) ? 2 * hcc + 16 * f2 : 3 * hcc + 16 * (f2 - HT);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (HALF && f2 % HT == HT - 1 && r >= 2) continue;   // k-steps of padding rows only
                    aj0 = mfma4(Wc0[(rb + rho16(0, r)) * LROW], zr[f2][r], aj0);
                    if (!HB) aj1 = mfma4(Wc1[(rb + rho16(0, r)) * LROW], zr[f2][r], aj1);
                }
            }
        };
        // u, v partial rows of one chunk += Ws[chunk] a, Wp[chunk] l for one gene block
        auto p1 = [&](const float *Wb, int hcc, const float *av, const float *lv, f32x4 (&acc)[F2]) {
            const float *Wr = Wb + offR_ + goff;
#pragma unroll
            for (int j = 0; j < GW; ++j) {
#pragma unroll
                for (int f = 0; f < HT; ++f) {
                    acc[f] = mfma4(Wr[f * 16 * LROW + j], av[j], acc[f]);
                    acc[HT + f] = mfma4(Wr[(hcc + f * 16) * LROW + j], lv[j], acc[HT + f]);
                }
            }
        };
        auto publish = [&](int ttl, int ch, f32x4 (&acc)[F2]) {
            const int pb = (gt * R * 64 + (ttl * NPT + ch * F2 * 2) * 128) * 8;   // this member's pairs of (tile, chunk)
#pragma unroll
            for (int f = 0; f < F2; ++f) {
                st_pair(prs, pb + (f * 2 + 0) * 1024, acc[f][0], acc[f][1], tagOut);
                if (pair_live(f * 2 + 1)) st_pair(prs, pb + (f * 2 + 1) * 1024, acc[f][2], acc[f][3], tagOut);
            }
        };
        // Half-block tiles with spare waves (ntg <= NW / 2): the nh = NW / ntg - 1 HELPER waves of a tile take hidden chunks off
        // its owner -- phase A's partial sums come back through LDS, phase F's activations go out through LDS (one barrier each)
        const int nh = HB ? d.NW / ntg - 1 : 0;
        const bool hs = HB && nh > 0;
        const int wt = hs ? wv % ntg : 0, wm = hs ? wv / ntg : 0;   // this wave's tile and member index (0: the owner)
        // Block split (one-slot instantiation on multi-block gene tiles, d.split parts): wave w works on block w / ntg of tile
        // w mod ntg in all three phases; what the blocks of a tile SUM -- the partial hidden rows, the norm partials -- is added
        // in LDS in part order before part 0 publishes (two barriers per publication).  k1_solve_fwd3's SPLIT, per chunk.
        const int nsp = (NBT == 1 && !HB) ? d.split : 1;
        const bool sp = nsp > 1;
        const int spt = sp ? wv % ntg : 0, spp = sp ? wv / ntg : 0;
        float *spc = hsP;   // (the hand-over region of the half-block form: the two forms exclude each other)
        auto slot_ok = [&](int i, int &s, int &bl, int &ttl) -> bool {   // slot i of this wave = (tile s, block bl)
            if (sp) { s = 0; bl = spp; ttl = spt; return spp < nsp && bl < nbl; }
            s = i >> lnb; bl = i & (d.NB - 1); ttl = hs ? wt : wv * d.TPW + s;
            return s < d.TPW && ttl < ntg && bl < nbl && wm <= nh;
        };
        // every wave of the workgroup calls this (two barriers); `nr` = norm partial of this wave's block (or nullptr)
        auto publish_split = [&](bool live, int ttl, int ch, f32x4 (&acc)[F2], bool rows, float *nr, unsigned int tagNn) {
            const int ent = ((spp - 1) * ntg + ttl) * (F2 * 256 + 64);
            if (live && spp > 0) {
                if (rows) {
#pragma unroll
                    for (int f = 0; f < F2; ++f) *reinterpret_cast<f32x4 *>(spc + ent + (f * 64 + lane) * 4) = acc[f];
                }
                if (nr) spc[ent + F2 * 256 + lane] = *nr;
            }
            __syncthreads();
            if (live && spp == 0) {
                for (int q = 1; q < nsp && q < nbl; ++q) {
                    const int eq = ((q - 1) * ntg + ttl) * (F2 * 256 + 64);
                    if (rows) {
#pragma unroll
                        for (int f = 0; f < F2; ++f) acc[f] += *reinterpret_cast<const f32x4 *>(spc + eq + (f * 64 + lane) * 4);
                    }
                    if (nr) *nr += spc[eq + F2 * 256 + lane];
                }
                if (rows) publish(ttl, ch, acc);
                if (nr) st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane, *nr, tagNn);
            }
            __syncthreads();
        };
        auto a_mine = [&](int ch) -> bool { return !hs || (ch + 1) % (nh + 1) == wm; };        // phase A: chunks 0 .. HC-2
        auto c_mine = [&](int ch) -> bool { return !hs || (HC - 1 - ch) % (nh + 1) == wm; };   // phase C: chunks HC-1 .. 0

        // ---- phase A: expansion partial sums of chunks 0 .. HC-2
        if (DO2) {
#pragma unroll
            for (int i = 0; i < NBT; ++i) { pj[i][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; pj[i][1] = pj[i][0]; }
            for (int ch = 0; ch + 1 < HC; ++ch) {
                ensure_chunk(ch, 11);
                prefetch(ch + 1);   // the next chunk of this phase, or phase F's (the last one)
                const int hcc = hc_of(ch);
                const float *Wch = lds + (long long)ch * cstr;
#pragma unroll
                for (int i = 0; i < NBT; ++i) {
                    int s, bl, ttl;
                    if (!slot_ok(i, s, bl, ttl) || !a_mine(ch)) continue;
                    if (bl == 0 || sp) gather(ttl, ch, tagIn);
                    p2(Wch + (long long)bl * BLKF_, hcc, pj[i][0], pj[i][1]);
                }
            }
            if (hs) {
                if (wm > 0 && wm <= nh) *reinterpret_cast<f32x4 *>(hsP + (wv * 64 + lane) * 4) = pj[0][0];
                __syncthreads();
                if (wm == 0)
                    for (int m = 1; m <= nh; ++m) {
                        const f32x4 o = *reinterpret_cast<const f32x4 *>(hsP + ((wt + m * ntg) * 64 + lane) * 4);
                        pj[0][0] += o;
                    }
            }
            tm.mark(11);
        }

        // ---- phase F: the narrow kernel's fused visit with the last chunk
        ensure_chunk(HC - 1, DO2 ? 11 : 0);
        if (DO1 && HC > 1) prefetch(HC - 2);   // phase C's first chunk flies under this phase (the forward kernel has the registers)
        {
            const int chL = HC - 1, hcL = hc_of(chL);
            const float *WchL = lds + (long long)chL * cstr;
            // per-tile state (set by the visit of the tile's first block)
            int lb = 0, b = 0, kb = 0;
            float sg = 1.f;
            float cin[6], cout[7], cer[7];
            f32x4 acc[F2];
            float r0 = 0.f, r1 = 0.f;
            float ty0[GW], tk[NKL][GW];
            bool liveF = false;
            auto issue = [&](int ttl, int bl) {
                tload<GW>(trs, lane32, toff(FC_Y0, ttl, bl), ty0);
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    if (SK1 && j == 1) {
#pragma unroll
                        for (int q = 0; q < GW; ++q) tk[j][q] = 0.f;
                    } else tload<GW>(trs, lane32, toff(FC_K + ring(kb, j), ttl, bl), tk[j]);
                }
            };
#pragma unroll
            for (int i = 0; i < NBT; ++i) {
                int s, bl, ttl;
                if (!slot_ok(i, s, bl, ttl) || wm != 0) continue;
                liveF = true;
                if (bl == 0 || sp) {
                    lb = ttl * 16 + li;
                    b = rowof(lb);
                    kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
                    issue(ttl, sp ? bl : 0);   // before the hidden rows are waited for: the tile latency overlaps the poll
                    if (DO2) { gather(ttl, chL, tagIn); tm.mark(4); }
                    sg = c.sgn[lb];
                    const float dtl = (cmode == 1) ? c.h0f[lb] : ((cmode == 2) ? c.dtf[lb] : 0.f);
#pragma unroll
                    for (int j = 0; j < 6; ++j) cin[j] = 0.f;
#pragma unroll
                    for (int j = 0; j < 7; ++j) { cout[j] = 0.f; cer[j] = 0.f; }
                    if (cmode == 1) { cin[0] = dtl; cout[0] = dtl; }
                    else if (cmode == 2) {
#pragma unroll
                        for (int j = 0; j < NK; ++j) cin[j] = DP_BETA[NK > 0 ? NK - 1 : 0][j] * dtl;
                        if (DO1) {
                            constexpr int ROW = DO2 ? NK : (NK >= 1 ? NK - 1 : 0);
                            constexpr int NT = DO2 ? NK + 1 : NK;
#pragma unroll
                            for (int j = 0; j < NT; ++j) cout[j] = DP_BETA[ROW < 6 ? ROW : 5][j] * dtl;
                        }
                        if (RM == 3) {
#pragma unroll
                            for (int j = 0; j < 7; ++j) cer[j] = dtl * DP_CERR[j];
                        }
                    }
#pragma unroll
                    for (int f = 0; f < F2; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    r0 = 0.f; r1 = 0.f;
                }
                {   // ---- one gene block
                    const float *Wb = WchL + (long long)bl * BLKF_;
                    const float *rg = lds + (long long)bl * BLKF_ + RGOFF;   // relu(g): in every chunk image, slot 0 is always there
                    float rr[GW];
#pragma unroll
                    for (int j = 0; j < GW; ++j) rr[j] = rg[gmap(lq, goff + j)];
                    if constexpr (CLAMP) {
#pragma unroll
                        for (int j = 0; j < GW; ++j)
                            if (clamp_holds(cset, (blk0 + bl) * 32 + gmap(lq, goff + j))) rr[j] = 0.f;
                    }
                    // ---- 1. everything that needs the tiles
                    float ysI[GW], ysN[GW], y0c[GW], k0c[GW], ey[GW];
                    if (DO2) {
                        float sy[GW];
#pragma unroll
                        for (int j = 0; j < GW; ++j) sy[j] = 0.f;
#pragma unroll
                        for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                            for (int j = 0; j < GW; ++j) sy[j] += tk[kk][j] * cin[kk];
#pragma unroll
                        for (int j = 0; j < GW; ++j) ysI[j] = (NK > 0) ? ty0[j] + sy[j] : ty0[j];
                    }
                    if (DO1) {
#pragma unroll
                        for (int j = 0; j < GW; ++j) ysN[j] = 0.f;
#pragma unroll
                        for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                            for (int j = 0; j < GW; ++j) ysN[j] += tk[kk][j] * cout[kk];
                    }
                    if (RM == 3) {
#pragma unroll
                        for (int j = 0; j < GW; ++j) ey[j] = 0.f;
#pragma unroll
                        for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                            for (int j = 0; j < GW; ++j) ey[j] += tk[kk][j] * cer[kk];
                    }
#pragma unroll
                    for (int j = 0; j < GW; ++j) y0c[j] = ty0[j];
                    if (RM == 2) {
#pragma unroll
                        for (int j = 0; j < GW; ++j) k0c[j] = tk[0][j];
                    }
                    // ---- 2. the tile registers are free: request the next block's tiles (fenced: see k1_solve_adj3)
                    __builtin_amdgcn_sched_barrier(0);
                    if (bl + 1 < nbl && !sp) issue(ttl, bl + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    // ---- 3. finish the stage: P2 of the last chunk on top of phase A's partial sums, k
                    float kv[GW];
                    if (DO2) {
                        float jv[GW];
                        {
                            f32x4 aj0 = pj[i][0], aj1 = pj[i][1];
                            p2(Wb, hcL, aj0, aj1);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                jv[r] = aj0[r];
                                if (!HB) jv[(GW - 4) + r] = aj1[r];
                            }
                        }
#pragma unroll
                        for (int j = 0; j < GW; ++j) kv[j] = sg * (rr[j] * (jv[j] - ysI[j]));
                        if (STK) tstore<GW>(trs, lane32, toff(FC_K + ring(kb, NK), ttl, bl), kv);
                        if (RM != 0) {
                            if (RM == 3) {
#pragma unroll
                                for (int j = 0; j < GW; ++j) ey[j] += kv[j] * cer[6];
                            }
#pragma unroll
                            for (int j = 0; j < GW; ++j) {
                                const int gene = (blk0 + bl) * 32 + gmap(lq, goff + j);
                                if (!((b < B) && (gene < N))) continue;
                                if (RM == 1) {
                                    const float scale = cfg.atol + fabsf(ysI[j]) * cfg.rtol;
                                    const float q0 = ysI[j] / scale, q1 = kv[j] / scale;
                                    r0 += q0 * q0; r1 += q1 * q1;
                                } else if (RM == 2) {
                                    const float scale = cfg.atol + fabsf(y0c[j]) * cfg.rtol;
                                    const float q0 = (kv[j] - k0c[j]) / scale;
                                    r0 += q0 * q0;
                                } else {
                                    const float tol = cfg.atol + cfg.rtol * fmaxf(fabsf(y0c[j]), fabsf(ysI[j]));
                                    const float q0 = ey[j] / tol;
                                    r0 += q0 * q0;
                                }
                            }
                        }
                    }
                    // ---- 4. next stage: input, activations (kept for phase C), P1 of the last chunk
                    if (DO1) {
                        float yn8[GW];
#pragma unroll
                        for (int j = 0; j < GW; ++j) {
                            if (DO2) yn8[j] = y0c[j] + (ysN[j] + kv[j] * cout[NK]);
                            else if (NK > 0) yn8[j] = y0c[j] + ysN[j];
                            else yn8[j] = y0c[j];
                        }
                        float av[GW], lv[GW];
                        act_pair_fast_pk<GW / 2>(yn8, av, lv);   // no masks: see k1_solve_fwd3
#pragma unroll
                        for (int j = 0; j < GW; ++j) { avq[i][j] = av[j]; avq[i][GW + j] = lv[j]; }
                        if (!hs) p1(Wb, hcL, av, lv, acc);
                        else {   // every chunk's contraction runs in phase C, split over the tile's waves
#pragma unroll
                            for (int j = 0; j < 2 * GW; ++j) hsA[(wt * 2 * GW + j) * 64 + lane] = avq[i][j];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (bl == nbl - 1 && !sp) {
                    if (DO1 && !hs) publish(ttl, chL, acc);
                    if (RM != 0) {
                        r0 = sum_over_q(r0); r1 = sum_over_q(r1);
                        st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane, lq == 0 ? r0 : (lq == 1 ? r1 : 0.f), tagN);
                    }
                }
            }
            if (sp && (DO1 || RM != 0)) {
                float nrv = 0.f;
                if (RM != 0 && liveF) { r0 = sum_over_q(r0); r1 = sum_over_q(r1); nrv = lq == 0 ? r0 : (lq == 1 ? r1 : 0.f); }
                publish_split(liveF, spt, chL, acc, DO1, RM != 0 ? &nrv : nullptr, tagN);
            }
        }
        tm.mark(DO2 ? (DO1 ? 2 : 5) : 1);

        // ---- phase C: contractions of chunks HC-2 .. 0 from the kept activations
        if (DO1) {
            if (hs) {
                __syncthreads();
                if (wm > 0 && wm <= nh) {
#pragma unroll
                    for (int j = 0; j < 2 * GW; ++j) avq[0][j] = hsA[(wt * 2 * GW + j) * 64 + lane];
                }
            }
            for (int ch = HC - (hs ? 1 : 2); ch >= 0; --ch) {
                ensure_chunk(ch, ch == HC - 2 ? (DO2 ? 2 : 1) : 12);
                if (ch > 0) prefetch(ch - 1);
                const int hcc = hc_of(ch);
                const float *Wch = lds + (long long)ch * cstr;
                f32x4 acc[F2];
#pragma unroll
                for (int i = 0; i < NBT; ++i) {
                    int s, bl, ttl;
                    const bool live = slot_ok(i, s, bl, ttl) && c_mine(ch);
                    if (live) {
                        if (bl == 0 || sp) {
#pragma unroll
                            for (int f = 0; f < F2; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        }
                        p1(Wch + (long long)bl * BLKF_, hcc, &avq[i][0], &avq[i][GW], acc);
                        if (bl == nbl - 1 && !sp) publish(ttl, ch, acc);
                    }
                    if (sp) publish_split(live, spt, ch, acc, true, nullptr, 0u);
                }
            }
            tm.mark(12);
        }
    };

    // ---- accept pass: dense output at the output times of this step (interp.py), advance, FSAL
    auto accept_pass = [&]() {
        const int lane32 = lane * 32 + 4 * goff;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;
            const int lb = ttl * 16 + li;
            const int b = rowof(lb);
            const int kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
            const bool rot = __builtin_amdgcn_readfirstlane(rotf[ttl]) != 0;
            const bool adv = !c.done[lb] && c.accept[lb];
            if (!__any(adv)) continue;
            const int lo = c.out_lo[lb], hi = c.out_hi[lb];
            const double t0 = c.rk_t0[lb], t1 = c.rk_t1[lb];
            const float dts = c.dtp[lb];
            const double sg = (double)c.sgn[lb];
            const TimeRow tb = trowT(t, T, cfg, shared ? trow_sh : min(b, B - 1));
            const bool outs = __any(adv && hi > lo);
            float y0A[GW], kA[7][GW], y0B[GW], kB[7][GW];
            auto request = [&](int bl, float(&y0v)[GW], float(&k)[7][GW]) {
                tload<GW>(trs, lane32, toff(FC_Y0, ttl, bl), y0v);
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    if (j == 1) {   // beta_72 = c_mid2 = 0
#pragma unroll
                        for (int q = 0; q < GW; ++q) k[j][q] = 0.f;
                    } else tload<GW>(trs, lane32, toff(FC_K + ring(kb, j), ttl, bl), k[j]);
                }
            };
            auto finish = [&](int bl, float(&y0v)[GW], float(&k)[7][GW]) {
                float y1v[GW], sy[GW];
#pragma unroll
                for (int j = 0; j < GW; ++j) sy[j] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 6; ++kk) {
                    const float cf = DP_BETA[5][kk] * dts;
#pragma unroll
                    for (int j = 0; j < GW; ++j) sy[j] += k[kk][j] * cf;
                }
#pragma unroll
                for (int j = 0; j < GW; ++j) y1v[j] = y0v[j] + sy[j];
                if (outs) {
                    float ym[GW];
#pragma unroll
                    for (int j = 0; j < GW; ++j) ym[j] = k[0][j] * (dts * DP_CMID[0]);
#pragma unroll
                    for (int kk = 1; kk < 6; ++kk) {
                        const float cf = dts * DP_CMID[kk];
#pragma unroll
                        for (int j = 0; j < GW; ++j) ym[j] += k[kk][j] * cf;
                    }
#pragma unroll
                    for (int j = 0; j < GW; ++j) ym[j] += k[6][j] * (dts * DP_CMID[6]);
                    if (adv) {
                        for (int jo = lo; jo < hi; ++jo) {
                            const double xx = (sg * tb[jo] - t0) / (t1 - t0);
                            const InterpX ix = make_interp_x(xx);
                            float ov[GW];
#pragma unroll
                            for (int j = 0; j < GW; ++j)
                                ov[j] = interp_eval(y0v[j], y1v[j], y0v[j] + ym[j], k[0][j], k[6][j], dts, ix);
                            row_storeG<GW>(sol, (long long)jo * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, goff), N, b < B,
                                       ov);
                        }
                    }
                }
                if (adv) {   // per-lane select: rejected / finished trajectories keep their state
                    tstore<GW>(trs, lane32, toff(FC_Y0, ttl, bl), y1v);
                    if (!rot) tstore<GW>(trs, lane32, toff(FC_K + kb, ttl, bl), k[6]);   // FSAL by copy (mixed decisions)
                }
            };
            request(0, y0A, kA);
            for (int bl = 0; bl < nbl; bl += 2) {
                if (bl + 1 < nbl) request(bl + 1, y0B, kB);
                __builtin_amdgcn_sched_barrier(0);
                finish(bl, y0A, kA);
                __builtin_amdgcn_sched_barrier(0);
                if (bl + 1 < nbl) {
                    if (bl + 2 < nbl) request(bl + 2, y0A, kA);
                    __builtin_amdgcn_sched_barrier(0);
                    finish(bl + 1, y0B, kB);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        tm.mark(10);
    };

    if (T >= 2) {
        float nv[2];
        {
            const unsigned int tH = ++x.tag;
            sweep(I3<0>{}, I3<0>{}, I3<1>{}, I3<0>{}, 0, 0u, tH, 0u);
            reduce_hidden();
            const unsigned int tN = ++x.tag;
            sweep(I3<0>{}, I3<1>{}, I3<0>{}, I3<1>{}, 0, tH, 0u, tN);
            norms(2, nv);   // d0, d1 (misc.py:62-67)
        }
        if (tid < Bt && !c.done[tid]) {
            c.h0f[tid] = init_h0(nv[0], nv[1]);
            c.d1[tid] = nv[1];
        }
        __syncthreads();
        {
            const unsigned int tH = ++x.tag;
            sweep(I3<1>{}, I3<0>{}, I3<1>{}, I3<0>{}, 1, 0u, tH, 0u);
            reduce_hidden();
            const unsigned int tN = ++x.tag;
            sweep(I3<1>{}, I3<1>{}, I3<0>{}, I3<2>{}, 1, tH, 0u, tN);
            norms(1, nv);
        }
        if (tid < Bt && !c.done[tid]) {
            const float h0 = c.h0f[tid];
            const float d2 = nv[0] / h0;
            const double dt = init_dt_ni(h0, c.d1[tid], d2);
            c.dt[tid] = dt; c.dtf[tid] = (float)dt; c.nfe[tid] = 2;
            const double t0 = c.rk_t1[tid];
            if (!(t0 + dt > t0)) { c.st[tid] = PHX_ERR_DT_UNDERFLOW; c.done[tid] = 1; }
        }
        int active = count_active();
        while (active > 0 && !x.aborted) {
            unsigned int tH = ++x.tag;
            sweep(I3<1>{}, I3<0>{}, I3<1>{}, I3<0>{}, 2, 0u, tH, 0u);
            reduce_hidden();
            {
                unsigned int tP = tH;
                tH = ++x.tag; sweep(I3<1>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<2>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<3>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<4>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<5>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                const unsigned int tN = ++x.tag;
                sweep(I3<6>{}, I3<1>{}, I3<0>{}, I3<3>{}, 2, tP, 0u, tN);
            }
            norms(1, nv);
            // ---- controller (rk_common.py:150-220)
            if (tid < Bt && !c.done[tid]) {
                const int lb = tid;
                const int b = rowof(lb);
                const TimeRow tb = trowT(t, T, cfg, shared ? trow_sh : b);
                const double sg = (double)c.sgn[lb];
                const float ratio = nv[0];
                const int acc = (ratio <= 1.0f) ? 1 : 0;
                const double t0 = c.rk_t1[lb], dt = c.dt[lb];
                c.rk_t0[lb] = t0;
                c.rk_t1[lb] = acc ? t0 + dt : t0;
                c.accept[lb] = acc;
                const int ns = c.nsteps[lb] + 1;
                c.nsteps[lb] = ns;
                c.nfe[lb] += 6;
                int oi = c.out_idx[lb];
                c.out_lo[lb] = oi;
                if (acc) {
                    const double t1 = t0 + dt;
                    while (oi < T && sg * tb[oi] <= t1) ++oi;
                }
                c.out_hi[lb] = oi;
                c.out_idx[lb] = oi;
                const double dtn = optimal_step_size_ni(dt, ratio);
                c.dtp[lb] = c.dtf[lb];
                c.dt[lb] = dtn;
                c.dtf[lb] = (float)dtn;
                // max_num_steps is a budget per output time (n_steps restarts in every _advance, rk_common.py:152-156)
                // and is tested before the step-size assert of the next step (rk_common.py:154,175)
                const int nsi = (oi > c.out_lo[lb]) ? 0 : c.nsiv[lb] + 1;
                c.nsiv[lb] = nsi;
                int dn = 0;
                if (oi >= T) dn = 1;
                else {
                    const double tn = c.rk_t1[lb];
                    if ((long long)nsi >= cfg.max_steps) { c.st[lb] = PHX_ERR_MAX_STEPS; dn = 1; }
                    else if (!(tn + dtn > tn)) { c.st[lb] = PHX_ERR_DT_UNDERFLOW; dn = 1; }
                }
                c.fin[lb] = dn;
            }
            __syncthreads();
            // the ring of a tile turns (k_7 -> k_1 without a copy) when every trajectory of it either continues with an
            // accepted step or is out after this step
            if (tid < ntg) {
                int ok = 1, cont = 0;
                for (int k = 0; k < 16; ++k) {
                    const int lb = tid * 16 + k;
                    const bool out = c.done[lb] || c.fin[lb] != 0;
                    const bool go = !c.done[lb] && c.accept[lb] && c.fin[lb] == 0;
                    if (!out && !go) ok = 0;
                    cont += go ? 1 : 0;
                }
                rotf[tid] = (ok && cont > 0) ? 1 : 0;
            }
            __syncthreads();
            tm.mark(9);
            accept_pass();
            __syncthreads();
            if (tid < ntg && rotf[tid]) kbs[tid] = ring(kbs[tid], 6);
            if (tid < Bt && !c.done[tid] && c.fin[tid]) c.done[tid] = 1;
            active = count_active();
        }
    }
    // ---- results (one workgroup per group reports)
    tm.mark(0);
    if (tm.on)
        for (int i = 0; i < 16; ++i) w.prof[(long long)blockIdx.x * 16 + i] = tm.acc[i];
    __syncthreads();
    // outputs a failed trajectory never reached are NaN (a backward solve launched on them stops at once)
    for (int s = 0; s < d.TPW; ++s) {
        const int ttl = wv * d.TPW + s;
        if (ttl >= ntg) continue;
        const int lb = ttl * 16 + li;
        const int b = rowof(lb);
        if (b < B && T >= 2 && (c.st[lb] != PHX_OK || x.aborted))
            for (int bl = 0; bl < nbl; ++bl)
                for (int jo = max(c.out_idx[lb], 1); jo < T; ++jo)
#pragma unroll
                    for (int j = 0; j < GW; ++j) {
                        const int gene = (blk0 + bl) * 32 + gmap(lq, goff + j);
                        if (gene < N) sol[(long long)jo * d.BN + (long long)b * N + gene] = __int_as_float(0x7fc00000);
                    }
    }
    if (gt == 0)
        for (int lb = tid; lb < Bt; lb += blockDim.x) {
            const int b = rowof(lb);
            if (b < B) {
                status[b] = x.aborted ? (int)PHX_ERR_SYNC_TIMEOUT : c.st[lb];
                nfe_out[b] = c.nfe[lb];
                nsteps_out[b] = c.nsteps[lb];
            }
        }
    xset_end(xs, grp, gt, G);
}

}  // namespace
