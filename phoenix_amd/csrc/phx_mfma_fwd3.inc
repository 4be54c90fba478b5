// phx_mfma_fwd3.inc -- third-generation forward solve: odeint(ODENet, y0, t) for dopri5 with a narrow hidden layer
// (H <= 48), the forward counterpart of k1_solve_adj3 (phx_mfma_adj3.inc).  Same algorithm, layouts, exchange protocol
// and controller arithmetic as k1_solve_fwd (phx_mfma_fwd.inc; reference: odeint.py, rk_common.py:39-228,
// misc.py:47-103, interp.py); what changed:
//   * 8 private vectors (Y0 and the ring of stage derivatives K[7]) instead of 9: a stage input is never stored, a sweep
//     recomputes it from Y0 and the k tiles it loads anyway (same fp32 operations in the same order);
//   * fused sweeps: one visit of a gene block finishes stage s (P2: j = W_alpha z, k_s) and forms stage s+1 (input,
//     activations, P1: u = Ws a, v = Wp l), stage number a compile-time constant, k_s consumed from registers;
//   * FSAL by turning the tile's ring of stage slots instead of copying k_7 -> k_1;
//   * private tiles addressed through a buffer resource (scalar tile offsets, one lane offset), no masks / branches in
//     the activations (a padding gene keeps y = 0.5, where a = l = 0, and zero weight columns);
//   * hidden rows exchanged as 16-byte granule pairs, a tile's rows gathered in one round trip;
//   * the accept pass (dense output at the output times, rk_common.py:168-196, interp.py) recomputes y1 from the tiles;
//   * a TERMINAL tile -- every running trajectory's candidate step reaches its last output time, so none of them takes
//     another step once it is accepted -- has no accept pass: its last-stage sweep holds Y0, k1, k3..k7 and y1 (the
//     recomputed stage input) in registers and writes the dense output from them; k7, y1 and the FSAL copy, which only a
//     further step would read, are not stored (a rejected trajectory repeats the step from untouched tiles and
//     overwrites the rows; a failed one has them NaN-filled from out_idx).
namespace {

enum { F_Y0 = 0, F_K = 1 };
constexpr int NVEC_FWD3 = 8;
constexpr int FWD3_NO_TERM = 0x100;   // W1::prof_level bit (prepare_fwd3, PHX_V3_TERM=0): no tile is marked terminal

// the controllers, kbs[ntg], rotf[ntg] and, in the 64 bytes behind them, termf[ntg] (ntg = NW * TPW <= 16: plan_fwd3)
__host__ __device__ inline size_t ctlf3_bytes(int Bt, int ntg) { return ctl_bytes(Bt) + (size_t)ntg * 8 + 64; }

// CALLS: the launch is d.TG independent odeint calls of d.Bcall rows under shared control (D1::Bcall, phx_solver.hpp):
// batch group g is call g, it reads time row g when cfg.t_per_sample is set, and the rows of its last tile beyond
// d.Bcall are padding (rowof).  A template flag, so that the instantiations of every other launch compile as before.
// CLAMP with CALLS: call g holds the genes clamp_gene[g * clamp_width .. + clamp_width) (at most PHX_CLAMP_MAX) at
// their initial values -- the sweeps read relu(g) of those genes as 0, so every stage slope of them is that of the model
// with g = 0 on the set (phx_odeint_clamped_sets); an index no gene has clamps nothing and pads a set.
// CLAMP without CALLS (phx_odeint_clamped_rows, per-trajectory control): the list is [B, clamp_width], one set per
// trajectory ROW; a lane masks with the set of its own trajectory (clamp_set_row), read at the head of every tile visit
// into four vector registers (the request flies under the wait for the hidden rows; the list, at most 16 bytes per row,
// stays in the L2) -- not staged in LDS, whose budget the planner shares with the forms that have no list.
// Without CLAMP the two trailing arguments are never read.
template <int HT, int MAXT, bool HALF, bool SPLIT, bool CALLS = false, bool CLAMP = false>
__global__ __launch_bounds__(MAXT) void k1_solve_fwd3(Net net, D1 d, W1 w, SolveCfg cfg, const float *__restrict__ y0,
                                                      const double *__restrict__ t, float *sol, int *status,
                                                      int *nfe_out, int *nsteps_out, const int *__restrict__ clamp_gene,
                                                      int clamp_width)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tile / row offsets stay scalar
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G;
    const bool shared = cfg.control == PHX_CTRL_SHARED;
    // the caller's row of local row lb (B: none, a padding row), and the time row of a shared-control group
    auto rowof = [&](int lb) -> int { return CALLS ? (lb < d.Bcall ? grp * d.Bcall + lb : B) : grp * Bt + lb; };
    const int trow_sh = CALLS ? grp : 0;
    ClampSet cset{};   // the call's held genes
    if constexpr (CLAMP && CALLS) cset = clamp_set(clamp_gene, grp, clamp_width);
    constexpr int F2 = 2 * HT;
    // small batches: the waves of a tile split its gene blocks (v3_split_parts, phx_mfma_v3common.inc)
    // (SPLIT is a template flag: the large-batch instantiation compiles exactly as without this path -- as run-time branches it cost
    // the C4 launch 0.8 % forward / 1.3 % backward through the register allocator's lottery)
    const int nparts = SPLIT ? v3_split_parts(d.TG, d.NW, d.TPW, ntg) : 1;
    const int wtile = SPLIT ? wv % ntg : wv * d.TPW;                 // the wave's first (split: only) trajectory tile
    const int part = SPLIT ? wv / ntg : 0;
    const int nbp = SPLIT ? (nbl + nparts - 1) / nparts : nbl;
    const int b_lo = SPLIT ? min(nbl, part * nbp) : 0, b_hi = SPLIT ? min(nbl, b_lo + nbp) : nbl;   // its gene blocks of the workgroup's tile
    // HALF: rows 8..15 of the last hidden tile are padding (rho16): k-steps 2, 3 / the second granule pair of that tile
    // carry nothing and are neither computed nor exchanged.  k = pair index inside a tile (f2, half); f2 = section tile.
    auto pair_live = [](int k) -> bool { return !(HALF && (k >> 1) % HT == HT - 1 && (k & 1)); };
    float *ctlbase = lds + (long long)d.NB * blk_floats_ch(HT, d.H);
    Ctl c = carve_ctl(ctlbase, Bt);
    int *kbs = reinterpret_cast<int *>(reinterpret_cast<char *>(ctlbase) + ctl_bytes(Bt));   // [ntg] ring base of the tile
    int *rotf = kbs + ntg;                                                                      // [ntg] ring turns now
    int *termf = rotf + ntg;   // [ntg] bit 0: the tile is terminal in the step under way, bit 1: in the one that follows
    float4 *comb = reinterpret_cast<float4 *>(reinterpret_cast<char *>(ctlbase) + ((ctlf3_bytes(Bt, ntg) + 15) & ~(size_t)15));
    const int RH = ntg * F2 * 4;   // hidden rows (u, v) of one exchange; norm rows follow
    const int R = RH + ntg;
    // this launch's set of exchange buffers (the other one is cleaned for the next launch: xset_begin)
    unsigned long long *xpart, *xzbuf;
    unsigned int *xabort;
    const XSet xs = xset_begin(w, grp, gt, G, R, xpart, xzbuf, xabort);
    Xchg x{xpart, xzbuf, 0, xabort, 0u, G, gt, R, false};
    // hidden rows travel in 16-byte PAIRS (see k1_solve_adj3): rows 2p, 2p + 1 interleaved per lane, a tag in each half
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
    const bool prof_sweep = (w.prof_level & 0xff) == 2;   // diagnostic: per-block timers inside the sweeps (slots 12..15)
    const bool fold = !(w.prof_level & FWD3_NO_TERM);

    // the first tile's initial state is requested before the weights are staged (its latency flies under the staging)
    constexpr int NBX = 8;   // plan_fwd3 never gives a workgroup more gene blocks
    float xinit[NBX][8];
    {
        const int ttl = wtile, b = rowof(ttl * 16 + li);
#pragma unroll
        for (int bl = 0; bl < NBX; ++bl)
            if (bl >= b_lo && bl < b_hi && ttl < ntg) row_load8(y0, (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B, 0.5f, xinit[bl]);
    }
    stage_images_flat(w.wimg, lds, blk0, nbl, blk_floats_ch(HT, d.H));

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
    for (int i = tid; i < ntg; i += blockDim.x) { kbs[i] = 0; rotf[i] = 0; termf[i] = 0; }
    // Terminal tiles (bit `bit` of termf): at least one trajectory of the tile runs and the candidate step of every
    // running one reaches its last output time -- `reach`, the controller's own comparison with t[T - 1].  Called by
    // whole waves where dt becomes known, thread lb with its trajectory's flags; a barrier that follows publishes it.
    auto mark_terminal = [&](int bit, bool run, bool reach) {
        const unsigned long long seg = 0xffffull << (lane & 48);   // the wave's lanes of this trajectory tile
        const unsigned long long mrun = __ballot(run) & seg, mshort = __ballot(run && !reach) & seg;
        if (tid < Bt && li == 0) termf[tid >> 4] = (termf[tid >> 4] & ~(1 << bit)) | ((fold && mrun && !mshort) ? 1 << bit : 0);
    };
    // ---- initial state: Y0 tiles <- y0, sol[0] <- y0
    {
        const int ttl = wtile, b = rowof(ttl * 16 + li);
#pragma unroll
        for (int bl = 0; bl < NBX; ++bl)
            if (bl >= b_lo && bl < b_hi && ttl < ntg) {
                const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                row_store8(sol, (long long)b * N, g0, N, b < B, xinit[bl]);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (g0 + j >= N) xinit[bl][j] = 0.5f;   // padding genes: a = l = 0
                bstore8(trs, lane * 32, toff(F_Y0, ttl, bl), xinit[bl]);
            }
    }
    for (int s = 1; s < d.TPW; ++s) {
        const int ttl = wtile + s;
        if (ttl >= ntg) continue;
        const int b = rowof(ttl * 16 + li);
        for (int bl = 0; bl < nbl; ++bl) {
            float xv[8];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
            row_load8(y0, (long long)b * N, g0, N, b < B, 0.5f, xv);
            row_store8(sol, (long long)b * N, g0, N, b < B, xv);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g0 + j >= N) xv[j] = 0.5f;   // padding genes: a = l = 0
            bstore8(trs, lane * 32, toff(F_Y0, ttl, bl), xv);
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
    auto poll_pairs = [&](auto NLc, int pr, int first, int step, int nv, float &s0, float &s1) {
        constexpr int NL = decltype(NLc)::value;   // member pairs in flight per lane (16, or 32 for groups of > 64 members)
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
        auto post = [&](int u, float tot) -> float {
            const int r = u & 3, f2 = (u >> 2) % F2;
            const int row = 16 * (f2 % HT) + rho16(lq, r);
            if (row >= d.H) return 0.f;
            return (f2 < HT) ? tot + net.bs[row] : expf(tot + net.bp[row]);
        };
        const int NP = RH / 2;
        if (G <= 16) {
            for (int p = gt + wv * G; p < NP; p += G * d.NW) {
                if (!pair_live(p % (F2 * 2))) continue;
                float s0, s1;
                poll_pairs(I3<16>{}, p, 0, 1, G, s0, s1);
                st_pair(zrs, p * 1024, post(2 * p, s0), post(2 * p + 1, s1), x.tag);
            }
        } else {
            for (int p = gt; p < NP; p += G) {
                if (!pair_live(p % (F2 * 2))) continue;   // workgroup uniform
                float s0 = 0.f, s1 = 0.f;
                // members g2, g2 + NW, ... of this wave, 16 per round trip (32 per round trip for groups of more than 64
                // members measured 3 % slower on 32..128-trajectory shards)
                for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                    int nv = 0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) nv += (g2 + k * d.NW < G) ? 1 : 0;
                    float a0, a1;
                    poll_pairs(I3<16>{}, p, g2, d.NW, nv, a0, a1);
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
            const int ttl = wtile + s;
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
    // One sweep over this wave's tiles (see k1_solve_adj3).  NK k tiles read; DO2: finish stage NK (gather its hidden
    // rows of exchange tagIn, recompute its input, P2, k_NK; RM 1: store k, norms d0 / d1; 2: no store, norm d2; 3: store
    // k, error ratio; 0: store k); DO1: form the next stage input, activations, P1 into exchange tagOut.
    // cmode 1: the single coefficient is h0, 2: dopri5 tableau rows.
    // -----------------------------------------------------------------------------------------------------------
    auto sweep = [&](auto NKc, auto D2c, auto D1c, auto RMc, int cmode, unsigned int tagIn, unsigned int tagOut,
                     unsigned int tagN) {
        constexpr int NK = decltype(NKc)::value;
        constexpr bool DO2 = decltype(D2c)::value != 0, DO1 = decltype(D1c)::value != 0;
        constexpr int RM = decltype(RMc)::value;
        constexpr bool STK = DO2 && RM != 2;
        constexpr bool SK1 = DO2 && !DO1 && NK == 6;   // last stage: beta_72 = c_err2 = 0, k_2 is not read
        constexpr bool FOLD = SK1 && RM == 3;          // ... of a step: a terminal tile takes the TERM bodies
        constexpr int NKL = NK > 0 ? NK : 1;
        tm.mark(0);
        // opaque copies: keeps the derived LDS / tile addresses of every sweep variant from being hoisted to the kernel top
        int H = d.H, BLKF = blk_floats_ch(HT, d.H), offR_ = offR, offC0 = offC[0], offC1 = offC[1], lane32 = lane * 32;
        asm volatile("" : "+s"(H), "+s"(BLKF));
        asm volatile("" : "+v"(offR_), "+v"(offC0), "+v"(offC1), "+v"(lane32));
        const int RGOFF = BLKF - 32;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wtile + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const int lb = ttl * 16 + li;
            const int b = rowof(lb);
            const int kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
            ClampSet rset{};   // the held genes of the lane's trajectory row
            if constexpr (CLAMP && !CALLS) rset = clamp_set_row(clamp_gene, b, B, clamp_width);
            const bool term = FOLD && (__builtin_amdgcn_readfirstlane(termf[ttl]) & 1);
            float ty0[8], tk[NKL][8];
            auto issue = [&](int bl) {
                bload8(trs, lane32, toff(F_Y0, ttl, bl), ty0);
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    if (SK1 && j == 1) zero8(tk[j]);
                    else bload8(trs, lane32, toff(F_K + ring(kb, j), ttl, bl), tk[j]);
                }
            };
            const bool has_blocks = !SPLIT || b_lo < b_hi;   // (split mode: the last gene tile may leave a part without a block)
            if (has_blocks) issue(b_lo);   // before the hidden rows are waited for: the tile latency overlaps the poll
            float zr[F2][4];
            if (DO2 && (!SPLIT || has_blocks)) {
                constexpr int NPT = F2 * 2;
                const int pb = ttl * NPT * 1024;
                i32x4 g[NPT];
#pragma unroll
                for (int k = 0; k < NPT; ++k) g[k] = pair_live(k) ? ld_pair(zrs, pb + k * 1024) : (i32x4){0, 0, 0, 0};
                unsigned int spins = 0;
                unsigned long long t_start = 0;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int k = 0; k < NPT; ++k)
                        ok = ok && (!pair_live(k) || ((unsigned int)g[k].y == tagIn && (unsigned int)g[k].w == tagIn));
                    if (__all(ok) || x.aborted) break;
                    __builtin_amdgcn_s_sleep(2);
#pragma unroll
                    for (int k = 0; k < NPT; ++k)
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
                for (int k = 0; k < NPT; ++k) {   // pair k = (f2, r >> 1): rows r = 2 (k & 1), + 1
                    zr[k >> 1][2 * (k & 1)] = __int_as_float(g[k].x);
                    zr[k >> 1][2 * (k & 1) + 1] = __int_as_float(g[k].z);
                }
                if (s == 0) tm.mark(4);
            }
            const float sg = c.sgn[lb];
            const float dtl = (cmode == 1) ? c.h0f[lb] : ((cmode == 2) ? c.dtf[lb] : 0.f);
            float cin[6], cout[7], cer[7];
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
            f32x4 acc[F2];
#pragma unroll
            for (int f = 0; f < F2; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float r0 = 0.f, r1 = 0.f;
            // a terminal tile's running trajectories (TERM bodies): the step and the output rows it would finish with
            bool live = false;
            int oi = T;
            double t0d = 0.0, t1d = 1.0, sgd = 1.0;
            TimeRow tb{t, false};
            if (term) {
                live = b < B && !c.done[lb];
                oi = c.out_idx[lb];
                t0d = c.rk_t1[lb]; t1d = t0d + c.dt[lb]; sgd = (double)sg;
                tb = trowT(t, T, cfg, shared ? trow_sh : min(b, B - 1));
            }
            auto body = [&](auto LASTc, auto TERMc, int bl) {
                constexpr bool LAST = decltype(LASTc)::value != 0;
                constexpr bool TERM = decltype(TERMc)::value != 0;   // only with FOLD: dense output instead of the k_7 store
                const float *Wb = lds + (long long)bl * BLKF;
                const float *rg = Wb + RGOFF;
                float rr[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) rr[j] = rg[gmap(lq, j)];
                if constexpr (CLAMP) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (clamp_holds(CALLS ? cset : rset, (blk0 + bl) * 32 + gmap(lq, j))) rr[j] = 0.f;
                }
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tm.mark(12); }   // diagnostic: tile wait
#endif
                // ---- 1. everything that needs the tiles
                float ysI[8], ysN[8], y0c[8], k0c[8], ey[8];
                if (DO2) {
                    float sy[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) sy[j] = 0.f;
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) sy[j] += tk[kk][j] * cin[kk];
#pragma unroll
                    for (int j = 0; j < 8; ++j) ysI[j] = (NK > 0) ? ty0[j] + sy[j] : ty0[j];
                }
                if (DO1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) ysN[j] = 0.f;
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) ysN[j] += tk[kk][j] * cout[kk];
                }
                if (RM == 3) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) ey[j] = 0.f;
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) ey[j] += tk[kk][j] * cer[kk];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) y0c[j] = ty0[j];
                if (RM == 2 || TERM) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) k0c[j] = tk[0][j];
                }
                float ym[8];
                if constexpr (TERM) {   // the dense output's midpoint combination as accept_pass forms it; k_7's term follows
#pragma unroll
                    for (int j = 0; j < 8; ++j) ym[j] = tk[0][j] * (dtl * DP_CMID[0]);
#pragma unroll
                    for (int kk = 1; kk < 6; ++kk) {
                        const float cf = dtl * DP_CMID[kk];
#pragma unroll
                        for (int j = 0; j < 8; ++j) ym[j] += tk[kk][j] * cf;
                    }
                }
                // ---- 2. the tile registers are free: request the next block's tiles (fenced: see k1_solve_adj3)
                __builtin_amdgcn_sched_barrier(0);
                if (!LAST) issue(bl + 1);
                __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep) tm.mark(13);   // diagnostic: consuming the tiles + requests
#endif
                // ---- 3. finish the stage: P2 and k  (f = relu(g) (W_alpha z - y), odenet.py:85-92)
                float kv[8];
                if (DO2) {
                    float jv[8];
                    {   // the two gene halves are independent accumulation chains: issued alternately, no MFMA waits for
                        // the result of the one before it (a dependent 16x16x4 f32 MFMA issues after 40 cycles, not 32)
                        f32x4 aj0 = (f32x4){0.f, 0.f, 0.f, 0.f}, aj1 = aj0;
                        const float *Wc0 = Wb + offC0, *Wc1 = Wb + offC1;
#pragma unroll
                        for (int f2 = 0; f2 < F2; ++f2) {
                            const int rb = (f2 < HT) ? 2 * H + 16 * f2 : 3 * H + 16 * (f2 - HT);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (HALF && f2 % HT == HT - 1 && r >= 2) continue;   // k-steps of padding rows only
                                aj0 = mfma4(Wc0[(rb + rho16(0, r)) * LROW], zr[f2][r], aj0);
                                aj1 = mfma4(Wc1[(rb + rho16(0, r)) * LROW], zr[f2][r], aj1);
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) { jv[r] = aj0[r]; jv[4 + r] = aj1[r]; }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) kv[j] = sg * (rr[j] * (jv[j] - ysI[j]));
                    if (STK && !TERM) bstore8(trs, lane32, toff(F_K + ring(kb, NK), ttl, bl), kv);
                    if (RM != 0) {
                        if (RM == 3) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) ey[j] += kv[j] * cer[6];
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int gene = (blk0 + bl) * 32 + gmap(lq, j);
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
                    if constexpr (TERM) {   // accept_pass's rows out_idx .. T - 1 from registers: y1 is this stage's input
#pragma unroll
                        for (int j = 0; j < 8; ++j) ym[j] += kv[j] * (dtl * DP_CMID[6]);
                        if (live) {
                            for (int jo = oi; jo < T; ++jo) {
                                const double xx = (sgd * tb[jo] - t0d) / (t1d - t0d);
                                const InterpX ix = make_interp_x(xx);
                                float ov[8];
#pragma unroll
                                for (int j = 0; j < 8; ++j)
                                    ov[j] = interp_eval(y0c[j], ysI[j], y0c[j] + ym[j], k0c[j], kv[j], dtl, ix);
                                row_store8(sol, (long long)jo * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, true, ov);
                            }
                        }
                    }
                }
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep && DO2) { __builtin_amdgcn_sched_barrier(0); tm.mark(14); }   // diagnostic: P2 + k + norms
#endif
                // ---- 4. next stage: input, activations, P1
                if (DO1) {
                    float av[8], lv[8], yn8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (DO2) yn8[j] = y0c[j] + (ysN[j] + kv[j] * cout[NK]);
                        else if (NK > 0) yn8[j] = y0c[j] + ysN[j];
                        else yn8[j] = y0c[j];
                    }
                    act_pair_fast8(yn8, av, lv);   // no masks: see the file header
                    const float *Wr = Wb + offR_;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
#pragma unroll
                        for (int f = 0; f < HT; ++f) {
                            acc[f] = mfma4(Wr[f * 16 * LROW + j], av[j], acc[f]);
                            acc[HT + f] = mfma4(Wr[(H + f * 16) * LROW + j], lv[j], acc[HT + f]);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep && DO1) tm.mark(15);   // diagnostic: next input + activations + P1
#endif
            };
            if (FOLD && term) {   // (wave uniform; a second instantiation of the block loop, no branch inside the bodies)
                if (has_blocks) {
                    for (int bl = b_lo; bl + 1 < b_hi; ++bl) body(I3<0>{}, I3<FOLD ? 1 : 0>{}, bl);
                    body(I3<1>{}, I3<FOLD ? 1 : 0>{}, b_hi - 1);
                }
            } else if (has_blocks) {
                for (int bl = b_lo; bl + 1 < b_hi; ++bl) body(I3<0>{}, I3<0>{}, bl);
                body(I3<1>{}, I3<0>{}, b_hi - 1);
            }
            if (SPLIT) {   // the tile's waves add their partial rows / norm partials in LDS, part 0 publishes
                float4 *mine = comb + (long long)wv * (F2 + 1) * 64 + lane;
                if (DO1) {
#pragma unroll
                    for (int f = 0; f < F2; ++f) mine[f * 64] = make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
                }
                if (RM != 0) mine[F2 * 64] = make_float4(r0, r1, 0.f, 0.f);
                __syncthreads();
                if (part == 0) {
                    for (int k = 1; k < nparts; ++k) {
                        const float4 *oth = comb + (long long)(ttl + k * ntg) * (F2 + 1) * 64 + lane;
                        if (DO1) {
#pragma unroll
                            for (int f = 0; f < F2; ++f) {
                                const float4 v = oth[f * 64];
                                acc[f][0] += v.x; acc[f][1] += v.y; acc[f][2] += v.z; acc[f][3] += v.w;
                            }
                        }
                        if (RM != 0) { const float4 v = oth[F2 * 64]; r0 += v.x; r1 += v.y; }
                    }
                }
                __syncthreads();   // the combine rows are free for the next sweep
            }
            if (DO1 && (!SPLIT || part == 0)) {
                const int pb = (gt * R * 64 + ttl * F2 * 2 * 128) * 8;   // this member's pairs of the tile
#pragma unroll
                for (int f = 0; f < F2; ++f) {
                    st_pair(prs, pb + (f * 2 + 0) * 1024, acc[f][0], acc[f][1], tagOut);
                    if (pair_live(f * 2 + 1)) st_pair(prs, pb + (f * 2 + 1) * 1024, acc[f][2], acc[f][3], tagOut);
                }
            }
            if (RM != 0 && (!SPLIT || part == 0)) {
                r0 = sum_over_q(r0); r1 = sum_over_q(r1);
                st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane, lq == 0 ? r0 : (lq == 1 ? r1 : 0.f), tagN);
            }
        }
        tm.mark(DO2 ? (DO1 ? 2 : 5) : 1);
    };

    // ---- accept pass: dense output at the output times of this step (interp.py), advance, FSAL
    auto accept_pass = [&]() {
        const int lane32 = lane * 32;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wtile + s;
            if (ttl >= ntg) continue;
            const int lb = ttl * 16 + li;
            const int b = rowof(lb);
            const int kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
            const bool rot = __builtin_amdgcn_readfirstlane(rotf[ttl]) != 0;
            if (__builtin_amdgcn_readfirstlane(termf[ttl]) & 1) continue;   // terminal: the last-stage sweep wrote its rows
            const bool adv = !c.done[lb] && c.accept[lb];
            if (!__any(adv)) continue;
            const bool keep = adv && !c.fin[lb];   // the trajectory takes another step: only then is its state read again
            const int lo = c.out_lo[lb], hi = c.out_hi[lb];
            const double t0 = c.rk_t0[lb], t1 = c.rk_t1[lb];
            const float dts = c.dtp[lb];
            const double sg = (double)c.sgn[lb];
            const TimeRow tb = trowT(t, T, cfg, shared ? trow_sh : min(b, B - 1));
            const bool outs = __any(adv && hi > lo);
            // two sets of tile registers: the next block's seven tiles are requested before this block's are consumed
            // (the loop is otherwise one exposed load latency per block: its stores may alias the next loads)
            float y0A[8], kA[7][8], y0B[8], kB[7][8];
            auto request = [&](int bl, float(&y0v)[8], float(&k)[7][8]) {
                bload8(trs, lane32, toff(F_Y0, ttl, bl), y0v);
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    if (j == 1) zero8(k[j]);   // beta_72 = c_mid2 = 0
                    else bload8(trs, lane32, toff(F_K + ring(kb, j), ttl, bl), k[j]);
                }
            };
            auto finish = [&](int bl, float(&y0v)[8], float(&k)[7][8]) {
                float y1v[8], sy[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) sy[j] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 6; ++kk) {
                    const float cf = DP_BETA[5][kk] * dts;
#pragma unroll
                    for (int j = 0; j < 8; ++j) sy[j] += k[kk][j] * cf;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) y1v[j] = y0v[j] + sy[j];
                if (outs) {
                    float ym[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) ym[j] = k[0][j] * (dts * DP_CMID[0]);
#pragma unroll
                    for (int kk = 1; kk < 6; ++kk) {
                        const float cf = dts * DP_CMID[kk];
#pragma unroll
                        for (int j = 0; j < 8; ++j) ym[j] += k[kk][j] * cf;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) ym[j] += k[6][j] * (dts * DP_CMID[6]);
                    if (adv) {
                        for (int jo = lo; jo < hi; ++jo) {
                            const double xx = (sg * tb[jo] - t0) / (t1 - t0);
                            const InterpX ix = make_interp_x(xx);
                            float ov[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j)
                                ov[j] = interp_eval(y0v[j], y1v[j], y0v[j] + ym[j], k[0][j], k[6][j], dts, ix);
                            row_store8(sol, (long long)jo * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B,
                                       ov);
                        }
                    }
                }
                if (keep) {   // per-lane select: rejected / finished trajectories keep their state
                    bstore8(trs, lane32, toff(F_Y0, ttl, bl), y1v);
                    if (!rot) bstore8(trs, lane32, toff(F_K + kb, ttl, bl), k[6]);   // FSAL by copy (mixed decisions)
                }
            };
            if (!SPLIT || b_lo < b_hi) request(b_lo, y0A, kA);
            for (int bl = b_lo; bl < b_hi; bl += 2) {
                if (bl + 1 < b_hi) request(bl + 1, y0B, kB);
                __builtin_amdgcn_sched_barrier(0);
                finish(bl, y0A, kA);
                __builtin_amdgcn_sched_barrier(0);
                if (bl + 1 < b_hi) {
                    if (bl + 2 < b_hi) request(bl + 2, y0A, kA);
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
        bool run = false, reach = false;
        if (tid < Bt && !c.done[tid]) {
            const float h0 = c.h0f[tid];
            const float d2 = nv[0] / h0;
            const double dt = init_dt_ni(h0, c.d1[tid], d2);
            c.dt[tid] = dt; c.dtf[tid] = (float)dt; c.nfe[tid] = 2;
            const double t0 = c.rk_t1[tid];
            if (!(t0 + dt > t0)) { c.st[tid] = PHX_ERR_DT_UNDERFLOW; c.done[tid] = 1; }
            else {
                const TimeRow tb = trowT(t, T, cfg, shared ? trow_sh : rowof(tid));
                run = true;
                reach = (double)c.sgn[tid] * tb[T - 1] <= t0 + dt;
            }
        }
        mark_terminal(0, run, reach);
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
            bool run = false, reach = false;   // of the step that follows (mark_terminal)
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
                    else { run = true; reach = sg * tb[T - 1] <= tn + dtn; }
                }
                c.fin[lb] = dn;
            }
            mark_terminal(1, run, reach);
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
            if (tid < ntg) termf[tid] >>= 1;   // the step that follows is now the step under way
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
        const int ttl = wtile + s;
        if (ttl >= ntg) continue;
        const int lb = ttl * 16 + li;
        const int b = rowof(lb);
        if (b < B && T >= 2 && (c.st[lb] != PHX_OK || x.aborted))
            for (int bl = b_lo; bl < b_hi; ++bl)
                for (int jo = max(c.out_idx[lb], 1); jo < T; ++jo)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int gene = (blk0 + bl) * 32 + gmap(lq, j);
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
