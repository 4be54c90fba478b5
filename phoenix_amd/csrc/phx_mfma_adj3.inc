// phx_mfma_adj3.inc -- third backward kernel of odeint_adjoint (dopri5, narrow hidden layer: H <= 48, the
// breast-cancer shape C4).  Same algorithm, decomposition, layouts, exchange protocol and controller arithmetic as
// k1_solve_adj (phx_mfma_adj.inc; reference: adjoint.py:32-162, rk_common.py:39-228, misc.py:47-103, interp.py);
// what changed is the BYTE STREAM of the private state (DESIGN.md "third backward kernel"):
//
//   * 16 private vectors instead of 37: Y0, A0 and the stage derivatives KY[7], KA[7].  Stage inputs are never
//     stored: a sweep that needs y_s / a_s recomputes them from Y0/A0 and the k tiles it loads anyway
//     (y_s = y0 + dt sum_j beta_sj k_j: the same fp32 operations in the same order as the pass that formed them).
//   * fused sweeps: one visit of a gene block finishes stage s (P2': expansion of the gathered hidden rows, k_s)
//     AND forms stage s+1 (input, activations, P1' contraction into the next exchange's partial rows), with the
//     stage number a compile-time constant; k_s is consumed from registers.
//   * the gene-multiplier term of the quadrature is derived from k_y (a * (j - y) = -sgn a k_y / relu(g)), so no
//     tile per stage is kept for it.
//   * the stage slots are a ring: when every running trajectory of a tile accepted its step the FSAL stage
//     (k_7 -> k_1, hidden rows included) is a change of the tile's ring base, not a copy.
//   * quadrature and accept pass share ONE visit per gene block: its 16 tiles are requested back to back (one
//     exposed latency per block instead of one per stage), all seven stage inputs are recomputed from them, the
//     parameter-gradient accumulators of the block stay in registers over the seven stages, and the dense-output /
//     jump / new (y0, a0) of the accept pass are formed from the same registers.
//
//   * the visit of the step that ends the solve can leave the kernel: a group whose trajectories all reach t_0 with the
//     first accepted step of the last interval writes their controller values into the head of its unwritten partial
//     and k3_tail_adj3 (phx_mfma_adj3_tail.inc), launched behind this kernel in place of k3_reduce_grads, runs the visit
//     on the whole chip (`deferred` below; DESIGN.md section 2).
//
// Tile passes (11.4 MB each at C4) per dopri5 step: sweeps 58 loads + 12 stores, quadrature + accept 16 + 2
// (k1_solve_adj: about 147).
namespace {

// (C_Y0, C_A0, C_KY, C_KA: the private vectors' slots, phx_mfma_v3common.inc -- k3_tail_adj3 reads them too)
constexpr int NVEC_ADJ3 = 16;

__host__ __device__ inline size_t ctl3_bytes(int Bt, int ntg)
{
    return ctl_bytes(Bt) + (size_t)Bt * 8 + (size_t)Bt * 8 * 4 + (size_t)ntg * 8 + 64 + 8192 /* pair combine */;
}


// grads (+)= sum over the wave partials of k1_solve_adj3 (accumulator-native order, see the kernel), fixed order =>
// deterministic.  One thread per (gene block, accumulator, lane): npart coalesced float4 loads, four scattered stores
// (rows 16 f + rho16(lq, r) of one gene); the tail threads sum dg, dbs, dbp.  Launched where the tail kernel is off
// (adj3_tail_on, phx_adj3t.hip: small launches, PHX_V3_TAIL=0); k3_tail_adj3 sums and writes the same way.
template <int HT>
__global__ __launch_bounds__(256) void k3_reduce_grads(const float *__restrict__ dtheta, int npart, long long PP, int N, int H,
                                                       int nblk, float *gWs, float *gWp, float *gWaT, float *gg, float *gbs,
                                                       float *gbp, int overwrite, float *gWa)
{
    constexpr int NA = 4 * HT * 2;
    const long long nq = (long long)nblk * NA * 64, og = nq * 4;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nq) {
        const int lane = (int)(tid & 63), a = (int)((tid >> 6) % NA), gb = (int)(tid / (NA * 64));
        const int li = lane & 15, lq = lane >> 4, s2 = a & 1, f = (a >> 1) % HT, m = (a >> 1) / HT;
        float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
        // eight partials requested at once, added in index order (the sum is the same as one at a time)
        int g = 0;
        for (; g + 8 <= npart; g += 8) {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = reinterpret_cast<const float4 *>(dtheta + (long long)(g + k) * PP)[tid];
#pragma unroll
            for (int k = 0; k < 8; ++k) { sacc.x += v[k].x; sacc.y += v[k].y; sacc.z += v[k].z; sacc.w += v[k].w; }
        }
        for (; g + 4 <= npart; g += 4) {   // (one partial per workgroup since round 4: npart = TG, 4 at C4)
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = reinterpret_cast<const float4 *>(dtheta + (long long)(g + k) * PP)[tid];
#pragma unroll
            for (int k = 0; k < 4; ++k) { sacc.x += v[k].x; sacc.y += v[k].y; sacc.z += v[k].z; sacc.w += v[k].w; }
        }
        for (; g < npart; ++g) {
            const float4 v = reinterpret_cast<const float4 *>(dtheta + (long long)g * PP)[tid];
            sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
        }
        const int gene = gb * 32 + gmapC(li, s2);
        float *dst = (m == 0) ? gWs : (m == 1 ? gWp : (m == 2 ? gWaT : gWaT + (long long)H * N));
        const float o[4] = {sacc.x, sacc.y, sacc.z, sacc.w};
        if (gWa && m >= 2) {
            // reference layout [N, 2H] (phx_grads.Wa): the lane's four values are hidden rows 16 f + rho16(lq, r) of one
            // gene (two pairs of neighbours), all inside one 64-byte stretch of the gene's row
            if (gene < N) {
                float *q = gWa + (long long)gene * 2 * H + (m - 2) * H + 16 * f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = rho16(lq, r);
                    if (16 * f + rr < H) q[rr] = overwrite ? o[r] : q[rr] + o[r];
                }
            }
        } else if (gene < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * f + rho16(lq, r);
                if (row < H) {
                    float *q = dst + (long long)row * N + gene;
                    *q = overwrite ? o[r] : *q + o[r];
                }
            }
        }
    } else {
        const long long e = tid - nq;   // dg [N], dbs [H], dbp [H]
        if (e < N + 2 * H) {
            float sacc = 0.f;
            for (int g = 0; g < npart; ++g) sacc += dtheta[(long long)g * PP + og + e];
            float *q = (e < N) ? gg + e : (e < N + H ? gbs + (e - N) : gbp + (e - N - H));
            *q = overwrite ? sacc : *q + sacc;
        }
    }
}

// CLAMP (phx_odeint_adjoint_backward_clamped_rows; the forms of phx_adj3r.hip): trajectory row b holds the genes
// clamp_gene[b * clamp_width .. + clamp_width) (at most PHX_CLAMP_MAX; an index no gene has pads a set) -- its adjoint
// is that of the model with g = 0 on the set.  A lane reads relu(g) of its trajectory's held genes as 0 wherever the
// multipliers enter: in the sweep body (vjp, k_y, q), and in the quadrature visit on q inside the trajectory-tile loop
// (the multipliers themselves are loaded once per half block, for all tiles).  dg needs no mask of its own: its term is
// a * k_y / relu(g) with the stored k_y, which the masked sweep left at 0 for a held gene.  The sets are read per tile
// visit into vector registers (clamp_set_row).  Without CLAMP the two trailing arguments are never read.
template <int HT, bool HALF, bool SPLIT, bool CLAMP = false>
__global__ __launch_bounds__(256) void k1_solve_adj3(Net net, D1 d, W1 w, SolveCfg cfg, const double *__restrict__ t,
                                                     const float *__restrict__ y_saved,
                                                     const float *__restrict__ grad_y, float *adj_y0, int *status,
                                                     int *nfe_out, int *nsteps_out, int want_grads_flags, long long PP,
                                                     const int *__restrict__ clamp_gene, int clamp_width)
{
    const int want_grads = want_grads_flags & 1;
    const bool prof_sweep = (want_grads_flags & 2) != 0, prof_quad = (want_grads_flags & 4) != 0;   // PHX_PROF=2 / 3
    // 8: the host launches k3_tail_adj3 behind this kernel -- a group whose trajectories all end the solve in its first
    // accepted step leaves that step's quadrature + accept visit to it (`deferred`, in front of quad_accept below)
    const bool may_defer = (want_grads_flags & 8) != 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    // wave-uniform by construction: telling the compiler keeps every tile / row base address in scalar registers
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, H = d.H, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G;
    const int BLKF = blk_floats_ch(HT, H);
    const int RGOFF = BLKF - 32;
    const bool shared = cfg.control == PHX_CTRL_SHARED;
    constexpr int F4 = 4 * HT, F2 = 2 * HT;
    // small batches: the waves of a tile split its gene blocks (v3_split_parts, phx_mfma_v3common.inc)
    // (SPLIT is a template flag: the large-batch instantiation compiles exactly as without this path)
    const int nparts = SPLIT ? v3_split_parts(d.TG, d.NW, d.TPW, ntg) : 1;
    const int wtile = SPLIT ? wv % ntg : wv * d.TPW;                 // the wave's first (split: only) trajectory tile
    const int part = SPLIT ? wv / ntg : 0;
    const int nbp = SPLIT ? (nbl + nparts - 1) / nparts : nbl;
    const int b_lo = SPLIT ? min(nbl, part * nbp) : 0, b_hi = SPLIT ? min(nbl, b_lo + nbp) : nbl;   // its gene blocks of the workgroup's tile
    // HALF: rows 8..15 of the last hidden tile are padding (rho16, phx_mfma_v3common.inc): k-steps 2, 3 of the products that
    // contract over hidden rows and the second granule pair of that tile in each of the four sections carry nothing and
    // are neither computed nor exchanged.  k = pair index inside a trajectory tile = (section tile f4) * 2 + half.
    auto pair_live = [](int k) -> bool { return !(HALF && (k >> 1) % HT == HT - 1 && (k & 1)); };
    float *ctlbase = lds + (long long)d.NB * BLKF;
    Ctl c = carve_ctl(ctlbase, Bt);
    double *xfin = reinterpret_cast<double *>(reinterpret_cast<char *>(ctlbase) + ctl_bytes(Bt));
    float *wq = reinterpret_cast<float *>(xfin + Bt);
    int *kbs = reinterpret_cast<int *>(wq + Bt * 8);   // [ntg] ring base of the tile's stage slots
    int *rotf = kbs + ntg;                             // [ntg] 1: the tile's ring turns at the end of this step
    float *wred3 = reinterpret_cast<float *>((reinterpret_cast<size_t>(rotf + ntg) + 63) & ~(size_t)63);   // [2][4][4][64]
    float4 *comb = reinterpret_cast<float4 *>(reinterpret_cast<char *>(ctlbase) + ((ctl3_bytes(Bt, ntg) + 15) & ~(size_t)15));
    const int RH = ntg * F4 * 4;   // hidden rows (u, v, dz_u, dz_p) of one exchange; norm rows follow
    const int R = RH + ntg;
    // this launch's set of exchange buffers (the other one is cleaned for the next launch: xset_begin)
    unsigned long long *xpart, *xzbuf;
    unsigned int *xabort;
    const XSet xs = xset_begin(w, grp, gt, G, R, xpart, xzbuf, xabort);
    Xchg x{xpart, xzbuf, 0, xabort, 0u, G, gt, R, false};
    // Hidden rows travel in PAIRS (rows 2p, 2p + 1 of a member's region interleaved per lane): one 16-byte sc1 access
    // moves two {tag, value} granules -- half the store / poll / gather instructions and half the reduce rounds of the
    // 8-byte form (8-byte sc1 accesses run at 0.54-0.70 of the 16-byte rate, MI355X_MICROARCH.md).  Each 8-byte half
    // still carries its own tag (only 8-byte halves are observed untorn).  Norm rows keep the 8-byte form.
    const __amdgpu_buffer_rsrc_t prs = make_rsrc(x.part, (unsigned int)((size_t)G * R * 512));
    const __amdgpu_buffer_rsrc_t zrs = make_rsrc(x.zbuf, (unsigned int)((size_t)R * 512));
    const int lane16x = lane * 16;
    auto st_pair = [&](__amdgpu_buffer_rsrc_t rs, int byte_off, float v0, float v1, unsigned int tag) {
        const i32x4 u = {__float_as_int(v0), (int)tag, __float_as_int(v1), (int)tag};
        store128<16>(u, rs, lane16x, byte_off);   // + the store-data hazard guard (phx_mfma_v3common.inc)
    };
    auto ld_pair = [&](__amdgpu_buffer_rsrc_t rs, int byte_off) -> i32x4 {
        // sc1 + the intrinsic's volatile bit: a poll must be re-issued on every pass and never sunk to its use
        return __builtin_amdgcn_raw_buffer_load_b128(rs, lane16x, byte_off, (int)0x80000010);
    };
    SegTimer tm;
    tm.start(w.prof != nullptr, c.tacc);
    const unsigned long long clk0 = tm.on ? (unsigned long long)clock64() : 0ull;   // diagnostic: shader clock

    // the first tile's terminal state (adjoint.py:86-87) is requested before the weights are staged (its latency flies
    // under the staging)
    constexpr int NBX = 8;   // plan_adj3 never gives a workgroup more gene blocks
    float xinit[NBX][8], ainit[NBX][8];
    {
        const int ttl = wtile, b = grp * Bt + ttl * 16 + li;
        const long long ro = (long long)(T - 1) * d.BN + (long long)b * N;
#pragma unroll
        for (int bl = 0; bl < NBX; ++bl)
            if (bl >= b_lo && bl < b_hi && ttl < ntg) {
                const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                row_load8(y_saved, ro, g0, N, b < B, 0.5f, xinit[bl]);
                row_load8(grad_y, ro, g0, N, b < B, 0.f, ainit[bl]);
            }
    }
    stage_images_flat(w.wimg, lds, blk0, nbl, BLKF);

    const int offR = rho16(li >> 2, li & 3) * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = rho16(lq, 0) * LROW + gmapC(li, 0);
    offC[1] = rho16(lq, 0) * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * d.nvec * tiles_wg * 512;
    const int lane8 = lane * 8;
    auto tptr = [&](int v, int ttl, int bl) -> float * {   // (uniform base) + 32-bit lane offset
        return wgbase + ((long long)v * tiles_wg + (ttl * d.NB + bl)) * 512 + lane8;
    };
    // the same tiles through a buffer resource: byte offset of tile (v, ttl, bl) in the workgroup's region
    const __amdgpu_buffer_rsrc_t trs = make_rsrc(wgbase, (unsigned int)(d.nvec * tiles_wg * 2048));
    auto toff = [&](int v, int ttl, int bl) -> int { return ((v * tiles_wg) + (ttl * d.NB + bl)) * 2048; };
    auto ring = [&](int kb, int j) -> int { const int v = kb + j; return v >= 7 ? v - 7 : v; };
    // reduced hidden rows of the running exchange: [grp][R][64] granules (one slot: an owner rewrites a row only after
    // every member has published the next exchange, i.e. after every member's wave of that tile has gathered this one)
    auto zrow = [&](int ttl, int f4, int r) -> u64 * {
        return x.zbuf + ((long long)(ttl * F4 + f4) * 4 + r) * 64;
    };
    // A stage's reduced hidden rows transposed for the products that contract over trajectories (xpose4), shared by the G
    // workgroups of the group: [group][tile][ring slot][F4 units][64 lanes] float4.  Unit (tile, f) is written ONCE per
    // stage, by the member (tile F4 + f) mod G when it gathers the rows (write-through stores, drained before that wave
    // publishes anything further); every member reads all units in its quadrature, behind an agent-scope acquire, with
    // plain loads: 1.3 MB at C4 that stay in the L2s instead of 81 MB of private copies streaming through the fabric.
    const __amdgpu_buffer_rsrc_t hrs = make_rsrc(w.hq + (long long)grp * ntg * 7 * (F4 * 256),
                                                 (unsigned int)(ntg * 7 * F4 * 1024));
    auto hoff = [&](int ttl, int slot, int f) -> int { return ((ttl * 7 + slot) * F4 + f) * 1024; };   // + 16 * lane
    // This wave's parameter-gradient partial, in ACCUMULATOR-NATIVE order: [gene block][4 HT x 2 accumulators][64 lanes]
    // float4 (accumulator (matrix m, hidden tile f, gene half s2) = (m HT + f) 2 + s2; lane (li, lq) component r <-> hidden
    // row 16 f + 4 lq + r, gene gmapC(li, s2) of the block), then dg [N], dbs [H], dbp [H].  Every store is a whole
    // 1 KB line-aligned chunk; k3_reduce_grads un-permutes while it sums the partials.
    float *dth = w.dtheta + (long long)grp * PP;       // ONE partial per workgroup (quad_accept: every slot has one owner wave)
    const long long og = (long long)d.nblk * (F4 * 2 * 256), obs = og + N, obp = obs + H;

    // ---- controllers
    for (int lb = tid; lb < Bt; lb += blockDim.x) {
        const int b = grp * Bt + lb;
        const bool vb = b < B;
        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : (vb ? b : 0));
        float sg = 1.0f;
        int st = PHX_OK;
        if (T >= 2) {
            sg = (tb[1] < tb[0]) ? -1.0f : 1.0f;
            for (int i = 0; i + 1 < T; ++i)
                if (!((double)sg * tb[i + 1] > (double)sg * tb[i])) st = PHX_ERR_BAD_ARG;
        }
        c.sgn[lb] = sg; c.st[lb] = vb ? st : PHX_OK; c.nsteps[lb] = 0; c.nfe[lb] = 0;
        c.done[lb] = (!vb || st != PHX_OK) ? 1 : 0;
        c.accept[lb] = 0; c.fin[lb] = 0; c.out_lo[lb] = 0;
        c.dtf[lb] = 0.f; c.h0f[lb] = 0.f; c.dtp[lb] = 0.f; c.d1[lb] = 0.f; c.dt[lb] = 0.0;
        xfin[lb] = 1.0;
        for (int j = 0; j < 8; ++j) wq[lb * 8 + j] = 0.f;
    }
    for (int i = tid; i < ntg; i += blockDim.x) { kbs[i] = 0; rotf[i] = 0; }
    // ---- terminal state (adjoint.py:86-87)
    {
        const int ttl = wtile;
#pragma unroll
        for (int bl = 0; bl < NBX; ++bl)
            if (bl >= b_lo && bl < b_hi && ttl < ntg) {
                store8(tptr(C_Y0, ttl, bl), xinit[bl]);
                store8(tptr(C_A0, ttl, bl), ainit[bl]);
            }
    }
    for (int s = 1; s < d.TPW; ++s) {
        const int ttl = wtile + s;
        if (ttl >= ntg) continue;
        const int b = grp * Bt + ttl * 16 + li;
        for (int bl = 0; bl < nbl; ++bl) {
            float xv[8], av[8];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
            const long long ro = (long long)(T - 1) * d.BN + (long long)b * N;
            row_load8(y_saved, ro, g0, N, b < B, 0.5f, xv);
            row_load8(grad_y, ro, g0, N, b < B, 0.f, av);
            store8(tptr(C_Y0, ttl, bl), xv);
            store8(tptr(C_A0, ttl, bl), av);
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

    // Reduce-scatter of rows [row0, row0 + nrows) of the current exchange (tag x.tag) by row ownership u mod G; the
    // reduced row u goes to zdst(u).  `comp(u)` names a second row reduced alongside (dv = dz_p * p needs the
    // matching v row), or -1.  Same three member layouts as k1_solve_adj.
    auto reduce_rows = [&](auto zdst, int row0, int nrows, auto comp, auto post) {
        if (G <= 16) {
            for (int u = gt + wv * G; u < nrows; u += G * d.NW) {
                const int row = row0 + u;
                const int crow = comp(u);
                const u64 *rows[16], *crows[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    rows[k] = x.part + ((long long)min(k, G - 1) * R + row) * 64;
                    crows[k] = x.part + ((long long)min(k, G - 1) * R + max(crow, 0)) * 64;
                }
                float v[16];
                wait_rows<16>(x, rows, G, lane, v);
                float tot = 0.f, ctot = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) tot += (k < G) ? v[k] : 0.f;
                if (crow >= 0) {
                    wait_rows<16>(x, crows, G, lane, v);
#pragma unroll
                    for (int k = 0; k < 16; ++k) ctot += (k < G) ? v[k] : 0.f;
                }
                st_gran(zdst(u), lane, post(u, tot, ctot), x.tag);
            }
            __syncthreads();
            return;
        }
        int wbuf = 0;
        for (int u = gt; u < nrows; u += G) {
            const int row = row0 + u;
            const int crow = comp(u);
            float sacc = 0.f, cacc = 0.f;
            for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                const u64 *rows[16], *crows[16];
                int nv = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int gg = g2 + k * d.NW;
                    rows[k] = x.part + ((long long)min(gg, G - 1) * R + row) * 64;
                    crows[k] = x.part + ((long long)min(gg, G - 1) * R + max(crow, 0)) * 64;
                    nv += (gg < G) ? 1 : 0;
                }
                float v[16];
                wait_rows<16>(x, rows, nv, lane, v);
#pragma unroll
                for (int k = 0; k < 16; ++k) sacc += (k < nv) ? v[k] : 0.f;
                if (crow >= 0) {
                    wait_rows<16>(x, crows, nv, lane, v);
#pragma unroll
                    for (int k = 0; k < 16; ++k) cacc += (k < nv) ? v[k] : 0.f;
                }
            }
            // combine through LDS, double buffered (NW <= 4: [buffer][row | companion][wave]): one barrier per row
            c.wred[(wbuf * 8 + wv) * 64 + lane] = sacc;
            c.wred[(wbuf * 8 + 4 + wv) * 64 + lane] = cacc;
            __syncthreads();
            if (wv == 0) {
                float tot = c.wred[wbuf * 8 * 64 + lane], ctot = c.wred[(wbuf * 8 + 4) * 64 + lane];
                for (int k = 1; k < d.NW; ++k) {
                    tot += c.wred[(wbuf * 8 + k) * 64 + lane];
                    ctot += c.wred[(wbuf * 8 + 4 + k) * 64 + lane];
                }
                st_gran(zdst(u), lane, post(u, tot, ctot), x.tag);
            }
            wbuf ^= 1;
        }
        __syncthreads();   // the combine buffers are free again; also the workgroup-wide "my rows are complete" point
    };

    // members' pairs [first + k step] of pair row `pr` until both halves of every one carry the tag; sums of the two rows
    // in member order
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
    // hidden exchange: reduce-scatter of the partial row PAIRS of the current exchange (tag x.tag) by pair ownership
    // p mod G; same member-to-wave assignment and summation order as reduce_rows
    auto reduce_hidden = [&]() {
        tm.mark(0);
        auto post = [&](int u, float tot) -> float {
            const int r = u & 3, f4 = (u >> 2) % F4;
            const int row = 16 * (f4 % HT) + rho16(lq, r);
            if (row >= H) return 0.f;
            if (f4 < HT) return tot + net.bs[row];
            if (f4 < F2) return expf(tot + net.bp[row]);
            return tot;                                     // du, dz_p (the members multiply dz_p by p when they gather)
        };
        const int NP = RH / 2;
        if (G <= 16) {
            for (int p = gt + wv * G; p < NP; p += G * d.NW) {
                if (!pair_live(p % (F4 * 2))) continue;
                float s0, s1;
                poll_pairs(I3<16>{}, p, 0, 1, G, s0, s1);
                st_pair(zrs, p * 1024, post(2 * p, s0), post(2 * p + 1, s1), x.tag);
            }
            __syncthreads();
        } else {
            int wbuf = 0;
            for (int p = gt; p < NP; p += G) {
                if (!pair_live(p % (F4 * 2))) continue;   // workgroup uniform
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
                // combine through LDS, double buffered ([buffer][s0 | s1][wave]): one barrier per pair
                float *wb = wred3 + wbuf * 1024;
                wb[(0 * 4 + wv) * 64 + lane] = s0; wb[(1 * 4 + wv) * 64 + lane] = s1;
                __syncthreads();
                if (wv == 0) {
                    float t2[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        t2[q] = wb[(q * 4) * 64 + lane];
                        for (int k = 1; k < d.NW; ++k) t2[q] += wb[(q * 4 + k) * 64 + lane];
                    }
                    st_pair(zrs, p * 1024, post(2 * p, t2[0]), post(2 * p + 1, t2[1]), x.tag);
                }
                wbuf ^= 1;
            }
            __syncthreads();   // the combine buffers are free again
        }
        tm.mark(3);
    };

    // ---- mixed Linf/RMS norm over the [y, a] blocks (misc.py:14-24): norm-row lanes (0,1) and (2,3)
    auto norms = [&](float *out2) {
        reduce_rows([&](int u) -> u64 * { return x.zbuf + (long long)(RH + u) * 64; }, RH, ntg,
                    [&](int) -> int { return -1; }, [&](int, float tot, float) -> float { return tot; });
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wtile + s;
            if (ttl >= ntg) continue;
            const u64 *rows[1] = {x.zbuf + (long long)(RH + ttl) * 64};
            float v[1];
            wait_rows<1>(x, rows, 1, lane, v);
            c.nrm[ttl * 64 + lane] = v[0];
        }
        __syncthreads();
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
        if (tid < Bt && (grp * Bt + tid) < B)
            for (int k = 0; k < 4; ++k) s4[k] = c.nrm[(tid >> 4) * 64 + k * 16 + (tid & 15)];
        double cnt = (double)N;
        if (shared) {
            if (tid < Bt) { c.tmpd[tid] = (double)s4[0]; c.tmpd[Bt + tid] = (double)s4[1]; }
            __syncthreads();
            double t0 = 0, t1 = 0;
            for (int lb = 0; lb < Bt; ++lb) { t0 += c.tmpd[lb]; t1 += c.tmpd[Bt + lb]; }
            __syncthreads();
            if (tid < Bt) { c.tmpd[tid] = (double)s4[2]; c.tmpd[Bt + tid] = (double)s4[3]; }
            __syncthreads();
            double t2 = 0, t3 = 0;
            for (int lb = 0; lb < Bt; ++lb) { t2 += c.tmpd[lb]; t3 += c.tmpd[Bt + lb]; }
            s4[0] = (float)t0; s4[1] = (float)t1; s4[2] = (float)t2; s4[3] = (float)t3;
            cnt = (double)d.BN;
        }
        __syncthreads();
        out2[0] = tmaxf(sqrtf((float)((double)s4[0] / cnt)), sqrtf((float)((double)s4[1] / cnt)));
        out2[1] = tmaxf(sqrtf((float)((double)s4[2] / cnt)), sqrtf((float)((double)s4[3] / cnt)));
        tm.mark(8);
    };

    // -----------------------------------------------------------------------------------------------------------
    // One sweep over this wave's tiles.  Compile-time shape:
    //   NK   k tiles per side read from memory (k_0 .. k_{NK-1} of the running step, ring relative)
    //   DO2  finish stage `NK`: gather its reduced hidden rows (exchange tagIn), recompute its input from the tiles,
    //        P2' (expansion back to genes), k_NK; RM: 1 = store k, norms d0/d1 (misc.py:62-67); 2 = no store, norm
    //        d2 (misc.py:74-77); 3 = store k, error ratio (rk_common.py:75-77, misc.py:89-91); 0 = store k
    //   DO1  form the next stage input (DO2: stage NK + 1, with k_NK from registers; else stage NK from the tiles),
    //        activations, P1' (contraction over genes) into the partial rows of exchange tagOut
    //   cmode 1: the single coefficient is h0 (second evaluation of _select_initial_step), 2: dopri5 tableau rows
    // -----------------------------------------------------------------------------------------------------------
    auto sweep = [&](auto NKc, auto D2c, auto D1c, auto RMc, int cmode, unsigned int tagIn, unsigned int tagOut,
                     unsigned int tagN, int flags = 0) {
        constexpr int NK = decltype(NKc)::value;
        constexpr bool DO2 = decltype(D2c)::value != 0, DO1 = decltype(D1c)::value != 0;
        constexpr int RM = decltype(RMc)::value;
        constexpr bool STK = DO2 && RM != 2;                 // k of the finished stage is stored
        constexpr bool SK1 = DO2 && !DO1 && NK == 6;         // last stage: beta_72 = c_err2 = 0, k_2 is not read
        constexpr int NKL = NK > 0 ? NK : 1;
        tm.mark(0);
        // Opaque copies of the inputs of the LDS / tile address arithmetic: without them every derived address of every
        // sweep variant is hoisted to the top of the kernel and lives (spilled) for its whole duration.
        int H = d.H, BLKF = blk_floats_ch(HT, d.H), offR_ = offR, offC0 = offC[0], offC1 = offC[1], lane32 = lane * 32, lane16 = lane * 16;
        asm volatile("" : "+s"(H), "+s"(BLKF));
        asm volatile("" : "+v"(offR_), "+v"(offC0), "+v"(offC1), "+v"(lane32), "+v"(lane16));
        const int RGOFF = BLKF - 32;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wtile + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const int lb = ttl * 16 + li;
            const int b = grp * Bt + lb;
            const int kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
            ClampSet rset{};   // the held genes of the lane's trajectory row
            if constexpr (CLAMP) rset = clamp_set_row(clamp_gene, b, B, clamp_width);
            bool hq_dirty = false;   // this wave wrote shared transposed rows: drained before its next publication
            float ty0[8], ta0[8], tky[NKL][8], tka[NKL][8];
            auto issue = [&](int bl) {
                bload8(trs, lane32, toff(C_Y0, ttl, bl), ty0);
                bload8(trs, lane32, toff(C_A0, ttl, bl), ta0);
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    if (SK1 && j == 1) { zero8(tky[j]); zero8(tka[j]); }
                    else {
                        bload8(trs, lane32, toff(C_KY + ring(kb, j), ttl, bl), tky[j]);
                        bload8(trs, lane32, toff(C_KA + ring(kb, j), ttl, bl), tka[j]);
                    }
                }
            };
            // the first block's tiles are requested BEFORE the hidden rows are waited for: their latency overlaps the poll
            const bool has_blocks = !SPLIT || b_lo < b_hi;   // (split mode: the last gene tile may leave a part without a block)
            if (has_blocks) issue(b_lo);
            float zr[F4][4];
            if (DO2 && (!SPLIT || has_blocks || part == 0)) {   // (part 0 gathers in any case: it writes the tile's shared transposed rows)
                const unsigned int keep = x.tag;
                x.tag = tagIn;
                // all F4 x 2 row pairs of the tile are requested back to back (one memory round trip when they are
                // complete); a batch of 8 pairs that is not complete yet is polled again on its own
                {
                    constexpr int NPT = F4 * 2, NBT = NPT / 8;
                    const int pb = ttl * NPT * 1024;
                    i32x4 g[NPT];
                    bool okb[NBT];
#pragma unroll
                    for (int k = 0; k < NPT; ++k) g[k] = pair_live(k) ? ld_pair(zrs, pb + k * 1024) : (i32x4){0, 0, 0, 0};
                    unsigned int spins = 0;
                    unsigned long long t_start = 0;
                    for (;;) {
                        bool all = true;
#pragma unroll
                        for (int bt = 0; bt < NBT; ++bt) {
                            bool ok = true;
#pragma unroll
                            for (int k = 0; k < 8; ++k)
                                ok = ok && (!pair_live(bt * 8 + k) ||
                                            ((unsigned int)g[bt * 8 + k].y == x.tag && (unsigned int)g[bt * 8 + k].w == x.tag));
                            okb[bt] = __all(ok);
                            all = all && okb[bt];
                        }
                        if (all || x.aborted) break;
                        __builtin_amdgcn_s_sleep(2);
#pragma unroll
                        for (int bt = 0; bt < NBT; ++bt)
                            if (!okb[bt]) {
#pragma unroll
                                for (int k = 0; k < 8; ++k)
                                    if (pair_live(bt * 8 + k)) g[bt * 8 + k] = ld_pair(zrs, pb + (bt * 8 + k) * 1024);
                            }
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
                    for (int k = 0; k < NPT; ++k) {   // pair k = (f, r >> 1): rows r = 2 (k & 1), + 1
                        zr[k >> 1][2 * (k & 1)] = __int_as_float(g[k].x);
                        zr[k >> 1][2 * (k & 1) + 1] = __int_as_float(g[k].z);
                    }
                    // dv = dz_p * p (p = exp(v + bp) = the z_p rows gathered alongside): formed here, by every member,
                    // instead of by the row's owner -- which would have to wait for a second (companion) row first
#pragma unroll
                    for (int f = 0; f < HT; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r) zr[3 * HT + f][r] *= zr[HT + f][r];
                }
                x.tag = keep;
                if (want_grads && RM != 2) {   // the quadrature's A operands of this stage (the h0 probe is no stage)
                    const int hs = ring(kb, NK);
                    // FSAL of the units this member owns when the tile's ring did not turn (first exchange of a step that
                    // follows a step with mixed decisions in the tile): stage 7 -> stage 1 for the trajectories that
                    // continue with an accepted step (component r of a lane <-> trajectory 4 lq + r).  Having gathered
                    // this exchange proves that every member has left the previous step's quadrature (the reader).
                    const bool fsal = (flags & 1) != 0 && NK == 1 && __builtin_amdgcn_readfirstlane(rotf[ttl]) == 0;
                    bool cp[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lbr = ttl * 16 + 4 * lq + r;
                        cp[r] = fsal && !c.done[lbr] && c.accept[lbr] && c.fin[lbr] == 0;
                    }
#pragma unroll
                    for (int f = 0; f < F4; ++f) {
                        if ((ttl * F4 + f) % G != gt || (SPLIT && part != 0)) continue;   // wave uniform: this member owns unit (tile, f)
                        float o[4];
                        xpose4(zr[f], o, lane);
                        bstore4_sc1(hrs, lane16, hoff(ttl, hs, f), o);
                        if (fsal) {
                            float v6[4], v0[4];
                            bload4_sc1(hrs, lane16, hoff(ttl, ring(kb, 6), f), v6);
                            bload4_sc1(hrs, lane16, hoff(ttl, kb, f), v0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v0[r] = cp[r] ? v6[r] : v0[r];
                            bstore4_sc1(hrs, lane16, hoff(ttl, kb, f), v0);
                        }
                        hq_dirty = true;
                    }
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
            f32x4 acc[F4];
#pragma unroll
            for (int f = 0; f < F4; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
            auto body = [&](auto LASTc, int bl) {
                constexpr bool LAST = decltype(LASTc)::value != 0;
                // (the PHXMARK comments are for tools/spill_map.py -- and they stay: as volatile asm they fence the scheduler, and
                // without them the launch is 1.3 % SLOWER: 0.5355 -> 0.5422 ms, round 4)
                asm volatile("; PHXMARK sweep NK=%0 DO2=%1 DO1=%2 RM=%3 LAST=%4" ::"n"(NK), "n"((int)DO2), "n"((int)DO1), "n"(RM), "n"((int)LAST));
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tm.mark(12); }   // diagnostic: tile wait
#endif
                const float *Wb = lds + (long long)bl * BLKF;
                const float *rg = Wb + RGOFF;
                float rr[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) rr[j] = rg[gmap(lq, j)];
                if constexpr (CLAMP) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (clamp_holds(rset, (blk0 + bl) * 32 + gmap(lq, j))) rr[j] = 0.f;
                }
                // ---- 1. everything that needs the tiles: stage inputs (rk_common.py:62-66), error partial, copies
                float ysI[8], asI[8], ysN[8], asN[8], y0c[8], a0c[8], k0y[8], k0a[8], ey[8], ea[8];
                if (DO2) {
                    float sy[8], sa[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { sy[j] = 0.f; sa[j] = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) { sy[j] += tky[kk][j] * cin[kk]; sa[j] += tka[kk][j] * cin[kk]; }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        ysI[j] = (NK > 0) ? ty0[j] + sy[j] : ty0[j];
                        asI[j] = (NK > 0) ? ta0[j] + sa[j] : ta0[j];
                    }
                }
                if (DO1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ysN[j] = 0.f; asN[j] = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) { ysN[j] += tky[kk][j] * cout[kk]; asN[j] += tka[kk][j] * cout[kk]; }
                }
                if (RM == 3) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ey[j] = 0.f; ea[j] = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                        for (int j = 0; j < 8; ++j) { ey[j] += tky[kk][j] * cer[kk]; ea[j] += tka[kk][j] * cer[kk]; }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) { y0c[j] = ty0[j]; a0c[j] = ta0[j]; }
                if (RM == 2) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { k0y[j] = tky[0][j]; k0a[j] = tka[0][j]; }
                }
                // ---- 2. the tile registers are free: request the next block's tiles; the two MFMA phases below cover them.
                // The scheduler is fenced on both sides: it otherwise moves the requests behind the first MFMA groups
                // and parts of the NEXT block's consumption in front of the last ones (exposing the load latency).
                __builtin_amdgcn_sched_barrier(0);
                if (!LAST) issue(bl + 1);
                __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep) tm.mark(13);   // diagnostic: consuming the tiles + requests
#endif
                // ---- 3. finish the stage: P2' and k
                float ky[8], ka[8];
                if (DO2) {
                    float jv[8], dap[8], dlp[8];
                    {   // the two gene halves are independent accumulation chains: issued alternately, so that no MFMA of
                        // the j chain waits for the result of the one before it (a dependent 16x16x4 f32 MFMA issues after
                        // 40 cycles, not 32); the order inside every chain is unchanged
                        f32x4 aj0 = (f32x4){0.f, 0.f, 0.f, 0.f}, aj1 = aj0, aa0 = aj0, aa1 = aj0, al0 = aj0, al1 = aj0;
                        const float *Wc0 = Wb + offC0, *Wc1 = Wb + offC1;
                        // (steps = the live k-steps of a section: four per hidden tile, two in a HALF section's last tile)
                        constexpr int SPS = HALF ? 4 * HT - 2 : 4 * HT;
                        mfma_steps<2 * SPS, 4, 2>(
                            [&](int s, float *w) {
                                const int f2 = (s / SPS) * HT + (s % SPS) / 4, r = (s % SPS) % 4;
                                const int rb = (f2 < HT) ? 2 * H + 16 * f2 : 3 * H + 16 * (f2 - HT);
                                w[0] = Wc0[(rb + rho16(0, r)) * LROW];
                                w[1] = Wc1[(rb + rho16(0, r)) * LROW];
                            },
                            [&](int s, const float *w) {
                                const int f2 = (s / SPS) * HT + (s % SPS) / 4, r = (s % SPS) % 4;
                                aj0 = mfma4(w[0], zr[f2][r], aj0);
                                aj1 = mfma4(w[1], zr[f2][r], aj1);
                            });
                        mfma_steps<SPS, 2, 4>(
                            [&](int s, float *w) {
                                const int f = s / 4, r = s % 4;
                                w[0] = Wc0[(16 * f + rho16(0, r)) * LROW];
                                w[1] = Wc0[(H + 16 * f + rho16(0, r)) * LROW];
                                w[2] = Wc1[(16 * f + rho16(0, r)) * LROW];
                                w[3] = Wc1[(H + 16 * f + rho16(0, r)) * LROW];
                            },
                            [&](int s, const float *w) {
                                const int f = s / 4, r = s % 4;
                                aa0 = mfma4(w[0], zr[F2 + f][r], aa0);
                                al0 = mfma4(w[1], zr[3 * HT + f][r], al0);
                                aa1 = mfma4(w[2], zr[F2 + f][r], aa1);
                                al1 = mfma4(w[3], zr[3 * HT + f][r], al1);
                            });
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            jv[r] = aj0[r]; dap[r] = aa0[r]; dlp[r] = al0[r];
                            jv[4 + r] = aj1[r]; dap[4 + r] = aa1[r]; dlp[4 + r] = al1[r];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float dj = jv[j] - ysI[j];
                        float da, dl;
                        act_grad_fast3(ysI[j], da, dl);
                        const float vjp = (dap[j] * da + dlp[j] * dl) - asI[j] * rr[j];
                        ky[j] = -sg * (rr[j] * dj);
                        ka[j] = sg * vjp;
                    }
                    if (STK) {
                        bstore8(trs, lane32, toff(C_KY + ring(kb, NK), ttl, bl), ky);
                        bstore8(trs, lane32, toff(C_KA + ring(kb, NK), ttl, bl), ka);
                    }
                    if (RM != 0) {
                        if (RM == 3) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) { ey[j] += ky[j] * cer[6]; ea[j] += ka[j] * cer[6]; }
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                            if (!((b < B) && (gene < N))) continue;
                            if (RM == 1) {
                                const float sy = cfg.atol + fabsf(ysI[j]) * cfg.rtol, sa = cfg.atol + fabsf(asI[j]) * cfg.rtol;
                                const float q0 = ysI[j] / sy, q1 = asI[j] / sa, q2 = ky[j] / sy, q3 = ka[j] / sa;
                                r0 += q0 * q0; r1 += q1 * q1; r2 += q2 * q2; r3 += q3 * q3;
                            } else if (RM == 2) {
                                const float sy = cfg.atol + fabsf(y0c[j]) * cfg.rtol, sa = cfg.atol + fabsf(a0c[j]) * cfg.rtol;
                                const float q0 = (ky[j] - k0y[j]) / sy, q1 = (ka[j] - k0a[j]) / sa;
                                r0 += q0 * q0; r1 += q1 * q1;
                            } else {
                                const float ty = cfg.atol + cfg.rtol * fmaxf(fabsf(y0c[j]), fabsf(ysI[j]));
                                const float ta = cfg.atol + cfg.rtol * fmaxf(fabsf(a0c[j]), fabsf(asI[j]));
                                const float q0 = ey[j] / ty, q1 = ea[j] / ta;
                                r0 += q0 * q0; r1 += q1 * q1;
                            }
                        }
                    }
                }
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep && DO2) { __builtin_amdgcn_sched_barrier(0); tm.mark(14); }   // diagnostic: P2' + k + norms
#endif
                // ---- 4. next stage: input, activations, P1'
                if (DO1) {
                    float av[8], lv[8], qv[8], yn8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float yn, an;
                        if (DO2) { yn = y0c[j] + (ysN[j] + ky[j] * cout[NK]); an = a0c[j] + (asN[j] + ka[j] * cout[NK]); }
                        else if (NK > 0) { yn = y0c[j] + ysN[j]; an = a0c[j] + asN[j]; }
                        else { yn = y0c[j]; an = a0c[j]; }
                        yn8[j] = yn;
                        qv[j] = an * rr[j];
                    }
                    // No masks: a padding gene keeps (y, a) = (0.5, 0) for the whole solve (its weight columns and
                    // relu(g) are zero in the LDS image: k_y = k_a = 0), where a(y) = l(y) = q = 0; a padding
                    // trajectory (finite: it never steps) only feeds its own MFMA column.
                    act_pair_fast8(yn8, av, lv);
                    const float *Wr = Wb + offR_;
                    mfma_steps<8, 1, F4>(
                        [&](int j, float *w) {
#pragma unroll
                            for (int f = 0; f < HT; ++f) {
                                w[f] = Wr[f * 16 * LROW + j];
                                w[HT + f] = Wr[(H + f * 16) * LROW + j];
                            }
#pragma unroll
                            for (int f = 0; f < F2; ++f) w[F2 + f] = Wr[((f < HT ? 2 * H + 16 * f : 3 * H + 16 * (f - HT))) * LROW + j];
                        },
                        [&](int j, const float *w) {
#pragma unroll
                            for (int f = 0; f < HT; ++f) {
                                acc[f] = mfma4(w[f], av[j], acc[f]);
                                acc[HT + f] = mfma4(w[HT + f], lv[j], acc[HT + f]);
                            }
#pragma unroll
                            for (int f = 0; f < F2; ++f) acc[F2 + f] = mfma4(w[F2 + f], qv[j], acc[F2 + f]);
                        });
                }
                __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS
                if (tm.on && prof_sweep && DO1) tm.mark(15);   // diagnostic: next input + activations + P1'
#endif
            };
            if (has_blocks) {
                for (int bl = b_lo; bl + 1 < b_hi; ++bl) body(I3<0>{}, bl);
                body(I3<1>{}, b_hi - 1);
            }
            asm volatile("; PHXMARK sweep end");
            if (SPLIT) {   // the tile's waves add their partial rows / norm partials in LDS, part 0 publishes
                float4 *mine = comb + (long long)wv * (F4 + 1) * 64 + lane;
                if (DO1) {
#pragma unroll
                    for (int f = 0; f < F4; ++f) mine[f * 64] = make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
                }
                if (RM != 0) mine[F4 * 64] = make_float4(r0, r1, r2, r3);
                __syncthreads();
                if (part == 0) {
                    for (int k = 1; k < nparts; ++k) {
                        const float4 *oth = comb + (long long)(ttl + k * ntg) * (F4 + 1) * 64 + lane;
                        if (DO1) {
#pragma unroll
                            for (int f = 0; f < F4; ++f) {
                                const float4 v = oth[f * 64];
                                acc[f][0] += v.x; acc[f][1] += v.y; acc[f][2] += v.z; acc[f][3] += v.w;
                            }
                        }
                        if (RM != 0) { const float4 v = oth[F4 * 64]; r0 += v.x; r1 += v.y; r2 += v.z; r3 += v.w; }
                    }
                }
                __syncthreads();   // the combine rows are free for the next sweep
            }
            // the shared transposed rows this wave wrote must have landed before anything it publishes from here on can
            // be observed (the readers order their loads behind LATER exchanges only)
            if (hq_dirty) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (DO1 && (!SPLIT || part == 0)) {
                const int pb = (gt * R * 64 + ttl * F4 * 2 * 128) * 8;   // this member's pairs of the tile
#pragma unroll
                for (int f = 0; f < F4; ++f) {
                    st_pair(prs, pb + (f * 2 + 0) * 1024, acc[f][0], acc[f][1], tagOut);
                    if (pair_live(f * 2 + 1)) st_pair(prs, pb + (f * 2 + 1) * 1024, acc[f][2], acc[f][3], tagOut);
                }
            }
            if (RM != 0 && (!SPLIT || part == 0)) {
                r0 = sum_over_q(r0); r1 = sum_over_q(r1); r2 = sum_over_q(r2); r3 = sum_over_q(r3);
                st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane,
                        lq == 0 ? r0 : (lq == 1 ? r1 : (lq == 2 ? r2 : r3)), tagN);
            }
        }
        tm.mark(DO2 ? (DO1 ? 2 : 5) : 1);
    };

    // -----------------------------------------------------------------------------------------------------------
    // Quadrature of the parameter gradient over the seven stages of an accepted step + accept pass, one visit per gene
    // block.  Weights wq (zero => stage skipped): h c_sol (ordinary step) or h W(x) (last step of an interval, where the
    // reference evaluates its quartic dense output); dtheta += sum_s w_s VJP_theta(stage s) is the reference's P-sized
    // augmented state (adjoint.py:86-87,127) integrated with the same step, never materialised per trajectory.
    //   dWs += (w du)^T a, dWp += (w dv)^T l, dWaT += (w z)^T q (MFMA, contraction over trajectories: operands
    //   transposed in registers), dg += w a (j - y), dbs += w du, dbp += w dv.
    // First touch of a wave's partial uses plain stores (no memset, no read); later steps read-add-store.
    // -----------------------------------------------------------------------------------------------------------
    bool gfirst = true;
    // Work split of this visit (round 4): a wave takes HALF gene blocks (bl, s2) = hb, hb = wave, wave + NW, ... and runs
    // ALL trajectory tiles of the group through them, tile after tile, into the same accumulators -- so the contraction of
    // a gradient element runs over the group's 16 ntg trajectories inside one wave, the workgroup writes ONE partial
    // (every accumulator slot has exactly one owner wave) and k3_reduce_grads sums TG partials instead of TG NW.  The
    // tiles of the other waves are read behind the workgroup barrier in front of this visit; the accept pass of a
    // (tile, half block) runs where its stage data sit.  Half blocks balance (2 nbl items over NW waves), the live
    // accumulators are 4 HT (not 8 HT) and a wave without a tile of its own (small batches) works like any other.
    auto quad_accept = [&](int iv) {
        tm.mark(0);
        int H = d.H, BLKF = blk_floats_ch(HT, d.H), lane32 = lane * 32, lane16 = lane * 16;
        asm volatile("" : "+s"(H), "+s"(BLKF));
        asm volatile("" : "+v"(lane32), "+v"(lane16));
        const int RGOFF = BLKF - 32;
        // the shared transposed hidden rows were written (write-through, drained) by other workgroups before exchanges this
        // wave has since completed: one agent-scope acquire, then plain (cacheable) loads
        if (want_grads) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // group-wide: does any trajectory carry a quadrature weight / advance in this step?
        bool any_w = false, any_adv = false;
        for (int ttl = 0; ttl < ntg; ++ttl) {
            const int lb = ttl * 16 + li;
            float wany = 0.f;
#pragma unroll
            for (int j = 0; j < 7; ++j) wany += fabsf(wq[lb * 8 + j]);
            any_w = any_w || __any(wany != 0.f);
            any_adv = any_adv || __any(!c.done[lb] && c.accept[lb]);
        }
        const bool wr_first = want_grads && gfirst;        // first visit: plain stores into the partial, no read
        const bool doq_g = want_grads && (any_w || wr_first);
        if (doq_g || any_adv)
        for (int hb = wv; hb < 2 * nbl; hb += d.NW) {
            const int bl = hb >> 1, s2 = hb & 1;
            const float *Wb = lds + (long long)bl * BLKF;
            const float *rg = Wb + RGOFF;
            const int gene0 = (blk0 + bl) * 32;
            const int lane32h = lane32 + 16 * s2;          // this gene half inside a lane's 32-byte tile slot
            float rr[4], rinv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rr[j] = rg[gmap(lq, 4 * s2 + j)];
                rinv[j] = rr[j] > 0.f ? fast_rcp(rr[j]) : 0.f;
            }
            f32x4 gs_[HT], gp_[HT], ga_[F2];
            float dgacc[4], sbias[HT], pbias[HT];
#pragma unroll
            for (int f = 0; f < HT; ++f) { gs_[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; gp_[f] = gs_[f]; sbias[f] = 0.f; pbias[f] = 0.f; }
#pragma unroll
            for (int f = 0; f < F2; ++f) ga_[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) dgacc[j] = 0.f;
            for (int ttl = 0; ttl < ntg; ++ttl) {
                const int lb = ttl * 16 + li;
                const int b = grp * Bt + lb;
                const int kb = __builtin_amdgcn_readfirstlane(kbs[ttl]);
                const bool adv = !c.done[lb] && c.accept[lb];
                const int fin = c.fin[lb];
                const bool rot = __builtin_amdgcn_readfirstlane(rotf[ttl]) != 0;
                float wn[7];
                float wany = 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) { wn[j] = wq[lb * 8 + j]; wany += fabsf(wn[j]); }
                const bool doq = doq_g && __any(wany != 0.f);
                if (!doq && !__any(adv)) continue;
                const float sg = c.sgn[lb];
                const float dts = c.dtp[lb];
                const InterpX ix = make_interp_x(xfin[lb]);
                const bool okb = b < B;
                int held = 0;   // bit j: this lane's trajectory holds gene j of the lane's four (q of it is 0)
                if constexpr (CLAMP) {
                    const ClampSet rset = clamp_set_row(clamp_gene, b, B, clamp_width);
#pragma unroll
                    for (int j = 0; j < 4; ++j) held |= clamp_holds(rset, gene0 + gmap(lq, 4 * s2 + j)) ? 1 << j : 0;
                }
                float y0v[4], a0v[4], ky[7][4], ka[7][4];
                bload4(trs, lane32h, toff(C_Y0, ttl, bl), y0v);
                bload4(trs, lane32h, toff(C_A0, ttl, bl), a0v);
                bload4(trs, lane32h, toff(C_KY + kb, ttl, bl), ky[0]);
                bload4(trs, lane32h, toff(C_KA + kb, ttl, bl), ka[0]);
                // transposed hidden rows of a stage: double buffered, the next stage's are requested a stage ahead
                float hA[F4][4], hB[F4][4];
                auto issue_h = [&](auto Pc, int S) {
                    constexpr int P = decltype(Pc)::value;
                    const int hs = ring(kb, S);
#pragma unroll
                    for (int f = 0; f < F4; ++f)   // du | dv first: they are used first
                        bload4(hrs, lane16, hoff(ttl, hs, (f + F2) % F4), P ? hB[f] : hA[f]);
                };
                if (doq) issue_h(I3<0>{}, 0);
#pragma unroll
                for (int j = 1; j < 7; ++j) {
                    bload4(trs, lane32h, toff(C_KY + ring(kb, j), ttl, bl), ky[j]);
                    bload4(trs, lane32h, toff(C_KA + ring(kb, j), ttl, bl), ka[j]);
                }
                float y1[4], a1[4];
                auto stage = [&](auto Sc) {
                    constexpr int S = decltype(Sc)::value;
                    constexpr int P = S & 1;
                    asm volatile("; PHXMARK quad stage %0" ::"n"(S));
                    if (doq && S < 6) issue_h(I3<1 - P>{}, S + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    // stage input, recomputed as the sweep formed it
                    float ys[4], as[4];
                    if (S == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) { ys[j] = y0v[j]; as[j] = a0v[j]; }
                    } else {
                        float sy[4], sa[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) { sy[j] = 0.f; sa[j] = 0.f; }
#pragma unroll
                        for (int kk = 0; kk < S; ++kk) {
                            const float cf = DP_BETA[S > 0 ? S - 1 : 0][kk] * dts;
#pragma unroll
                            for (int j = 0; j < 4; ++j) { sy[j] += ky[kk][j] * cf; sa[j] += ka[kk][j] * cf; }
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) { ys[j] = y0v[j] + sy[j]; as[j] = a0v[j] + sa[j]; }
                    }
                    if (S == 6) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) { y1[j] = ys[j]; a1[j] = as[j]; }
                    }
                    if (!doq) return;
                    const float wl = wn[S];
                    if (!__any(wl != 0.f)) return;
                    float w4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) w4[r] = wq[(ttl * 16 + 4 * lq + r) * 8 + S];
                    float an[4], ln[4], qn[4];
                    // no masks: padding genes hold (0.5, 0) with relu(g) = 0, padding trajectories have weight zero
                    act_pair_fast_pk<2>(ys, an, ln);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        qn[j] = (CLAMP && (held >> j & 1)) ? 0.f : as[j] * rr[j];
                        // a (j - y) from k_y = -sgn relu(g) (j - y)
                        const float sgv = as[j] * (-sg * ky[S][j] * rinv[j]);
                        dgacc[j] += wl * sgv;
                    }
                    // The step weight of trajectory 4 lq + r goes into the B operands (the A operands -- the transposed
                    // hidden rows -- then feed the matrix pipe untouched by vector instructions)
                    float at[4], lt[4], qt[4];
                    xpose4(an, at, lane);
                    xpose4(ln, lt, lane);
                    xpose4(qn, qt, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { at[r] *= w4[r]; lt[r] *= w4[r]; qt[r] *= w4[r]; }
                    // h[0 .. F2) = du | dv rows, h[F2 .. F4) = z_u | z_p rows: lane (li, lq), component r <-> hidden row
                    // 16 f + rho16(li) of trajectory 4 lq + r
                    float(&h)[F4][4] = *(P ? &hB : &hA);
#pragma unroll
                    for (int f = 0; f < HT; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            gs_[f] = mfma4(h[f][r], at[r], gs_[f]);
                            gp_[f] = mfma4(h[HT + f][r], lt[r], gp_[f]);
                        }
#pragma unroll
                    for (int f = 0; f < F2; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ga_[f] = mfma4(h[F2 + f][r], qt[r], ga_[f]);
                    if (gt == 0 && hb == 0) {   // bias gradients (gene independent): dbs += w du, dbp += w dv, read again
                        const int hs = ring(kb, S);
#pragma unroll
                        for (int f = 0; f < HT; ++f) {
                            float u[4], v[4];
                            bload4(hrs, lane16, hoff(ttl, hs, F2 + f), u);
                            bload4(hrs, lane16, hoff(ttl, hs, 3 * HT + f), v);
                            sbias[f] += ((w4[0] * u[0] + w4[1] * u[1]) + w4[2] * u[2]) + w4[3] * u[3];
                            pbias[f] += ((w4[0] * v[0] + w4[1] * v[1]) + w4[2] * v[2]) + w4[3] * v[3];
                        }
                    }
                };
                stage(I3<0>{}); stage(I3<1>{}); stage(I3<2>{}); stage(I3<3>{}); stage(I3<4>{}); stage(I3<5>{});
                float gy4[4], ys4[4];
                {   // jump data of the trajectories that reach t_{i-1} in this step (adjoint.py:152-154), requested in
                    // front of the last stage so that its work covers them: the lane's four genes of this gene half
                    const long long ro = (long long)(iv - 1) * d.BN + (long long)b * N;
                    const int g0 = gene0 + gmap(lq, 4 * s2);
                    row_load4(grad_y, ro, g0, N, okb && fin == 1, 0.f, gy4);
                    row_load4(y_saved, ro, g0, N, okb && fin == 1, 0.5f, ys4);
                }
                stage(I3<6>{});
                asm volatile("; PHXMARK accept");
                // ---- accept pass (rk_common.py:168-196; dense output interp.py:1-47; jump adjoint.py:152-154)
                if (__any(adv)) {
                    float am[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) am[j] = ka[0][j] * (dts * DP_CMID[0]);
#pragma unroll
                    for (int kk = 2; kk < 6; ++kk) {   // DP_CMID[1] == 0
                        const float cf = dts * DP_CMID[kk];
#pragma unroll
                        for (int j = 0; j < 4; ++j) am[j] += ka[kk][j] * cf;
                    }
                    float anew[4], ynew[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        am[j] += ka[6][j] * (dts * DP_CMID[6]);
                        if (fin == 1) {
                            const float aout = interp_eval(a0v[j], a1[j], a0v[j] + am[j], ka[0][j], ka[6][j], dts, ix);
                            anew[j] = aout + gy4[j];
                            ynew[j] = ys4[j];
                        } else {
                            anew[j] = a1[j];
                            ynew[j] = y1[j];
                        }
                    }
                    if (adv) {
                        bstore4(trs, lane32h, toff(C_A0, ttl, bl), anew);
                        bstore4(trs, lane32h, toff(C_Y0, ttl, bl), ynew);
                        if (fin != 1 && !rot) {   // FSAL by copy: the tile's ring does not turn (mixed decisions in the tile)
                            bstore4(trs, lane32h, toff(C_KA + kb, ttl, bl), ka[6]);
                            bstore4(trs, lane32h, toff(C_KY + kb, ttl, bl), ky[6]);
                        }
                    }
                }
            }
            asm volatile("; PHXMARK quad store");
            // ---- accumulators -> the workgroup's partial, as they stand in the registers (coalesced 16-byte accesses);
            // slot (matrix m, hidden tile f, gene half s2) of block bl has this wave as its only writer
            if (doq_g) {
                float4 *pn = reinterpret_cast<float4 *>(dth) + (long long)(blk0 + bl) * (F4 * 2 * 64) + lane;
                auto put = [&](int a, const f32x4 &v) {
                    float4 o = make_float4(v[0], v[1], v[2], v[3]);
                    if (!wr_first) {
                        const float4 old = pn[a * 64];
                        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
                    }
                    pn[a * 64] = o;
                };
#pragma unroll
                for (int f = 0; f < HT; ++f) {
                    put((0 * HT + f) * 2 + s2, gs_[f]);
                    put((1 * HT + f) * 2 + s2, gp_[f]);
                    put((2 * HT + f) * 2 + s2, ga_[f]);
                    put((3 * HT + f) * 2 + s2, ga_[HT + f]);
                }
                // dg: sum over the trajectories of a tile position (lanes with equal lq), one gene per register
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = dgacc[j];
                    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
                    const int gene = gene0 + gmap(lq, 4 * s2 + j);
                    if (li == 0 && gene < N) dth[og + gene] = (wr_first ? 0.f : dth[og + gene]) + v;
                }
                // bias gradients: gene independent => the first half block of the group's first gene tile carries them
                if (gt == 0 && hb == 0) {
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        float sb = sbias[f], sp = pbias[f];
                        sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
                        sp += __shfl_xor(sp, 16, 64); sp += __shfl_xor(sp, 32, 64);
                        const int hid = 16 * f + rho16(li >> 2, li & 3);   // the transposed rows' lane li holds this hidden row
                        if (lq == 0 && hid < H) {
                            dth[obs + hid] = (wr_first ? 0.f : dth[obs + hid]) + sb;
                            dth[obp + hid] = (wr_first ? 0.f : dth[obp + hid]) + sp;
                        }
                    }
                }
            }
        }
        if (doq_g) gfirst = false;
        tm.mark(10);
    };

    bool deferred = false;   // this group left its (only) visit to the tail kernel
    float nv[2];
    for (int iv = T - 1; iv >= 1; --iv) {
        // ---------------------------------------------------------------- dopri5 on [u0, u_end]
        __syncthreads();
        for (int lb = tid; lb < Bt; lb += blockDim.x) {
            const int b = grp * Bt + lb;
            if (b >= B || c.st[lb] != PHX_OK) { c.done[lb] = 1; continue; }
            const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
            const double sg = (double)c.sgn[lb];
            c.done[lb] = 0;
            c.rk_t0[lb] = -sg * tb[iv];
            c.rk_t1[lb] = -sg * tb[iv];
            c.accept[lb] = 0; c.fin[lb] = 0;
            c.out_lo[lb] = 0;   // max_num_steps is a per-interval budget (rk_common.py:152-156)
        }
        __syncthreads();
        // ---- _select_initial_step (misc.py:47-86): f0 = k_1 of the first step, then one evaluation at y0 + h0 f0
        {
            const unsigned int tH = ++x.tag;
            sweep(I3<0>{}, I3<0>{}, I3<1>{}, I3<0>{}, 0, 0u, tH, 0u);
            reduce_hidden();
            const unsigned int tN = ++x.tag;
            sweep(I3<0>{}, I3<1>{}, I3<0>{}, I3<1>{}, 0, tH, 0u, tN);
            norms(nv);   // d0 = norm(y0 / scale), d1 = norm(f0 / scale)
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
            norms(nv);
        }
        if (tid < Bt && !c.done[tid]) {
            const float h0 = c.h0f[tid];
            const float d2 = nv[0] / h0;
            const double dt = init_dt_ni(h0, c.d1[tid], d2);
            c.dt[tid] = dt; c.dtf[tid] = (float)dt; c.nfe[tid] += 2;
            const double t0 = c.rk_t1[tid];
            if (!(t0 + dt > t0)) { c.st[tid] = PHX_ERR_DT_UNDERFLOW; c.done[tid] = 1; }
        }
        int active = count_active();
        bool first_step = true;
        while (active > 0 && !x.aborted) {
            // ---- one dopri5 step: stage 1 is in the ring (FSAL / initial evaluation); six exchanges
            unsigned int tH = ++x.tag;
            sweep(I3<1>{}, I3<0>{}, I3<1>{}, I3<0>{}, 2, 0u, tH, 0u);
            reduce_hidden();
            {
                unsigned int tP = tH;
                tH = ++x.tag; sweep(I3<1>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u, first_step ? 0 : 1); reduce_hidden(); tP = tH;
                first_step = false;
                tH = ++x.tag; sweep(I3<2>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<3>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<4>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                tH = ++x.tag; sweep(I3<5>{}, I3<1>{}, I3<1>{}, I3<0>{}, 2, tP, tH, 0u); reduce_hidden(); tP = tH;
                const unsigned int tN = ++x.tag;
                sweep(I3<6>{}, I3<1>{}, I3<0>{}, I3<3>{}, 2, tP, 0u, tN);
            }
            norms(nv);
            if (tid < Bt && !c.done[tid]) {
                const int lb = tid;
                const int b = grp * Bt + lb;
                const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                const double sg = (double)c.sgn[lb];
                const double u_end = -sg * tb[iv - 1];
                const float ratio = nv[0];
                const int acc = (ratio <= 1.0f) ? 1 : 0;
                const double t0 = c.rk_t1[lb], dt = c.dt[lb];
                const double t1 = t0 + dt;
                c.rk_t0[lb] = t0;
                c.rk_t1[lb] = acc ? t1 : t0;
                c.accept[lb] = acc;
                c.nsteps[lb] += 1;
                const int ns = c.out_lo[lb] + 1;
                c.out_lo[lb] = ns;
                c.nfe[lb] += 6;
                const float dtf = c.dtf[lb];
                c.dtp[lb] = dtf;
                int fin = 0;
                double xx = 1.0;
                if (acc && u_end <= t1) { fin = 1; xx = (u_end - t0) / (t1 - t0); }
                xfin[lb] = xx;
                for (int j = 0; j < 8; ++j) {
                    float wj = 0.f;
                    if (acc && j < 7) {
                        double W;
                        if (!fin) W = DP_CSOL64[j];
                        else {
                            const double x2 = xx * xx, x3 = x2 * xx, x4 = x3 * xx;
                            const double d1 = (j == 0) ? 1.0 : 0.0, d7 = (j == 6) ? 1.0 : 0.0;
                            const double cj = DP_CSOL64[j], mj = DP_CMID64[j];
                            W = xx * d1 + x2 * (d7 - 4.0 * d1 - 5.0 * cj + 16.0 * mj) +
                                x3 * (5.0 * d1 - 3.0 * d7 + 14.0 * cj - 32.0 * mj) +
                                x4 * (2.0 * d7 - 2.0 * d1 - 8.0 * cj + 16.0 * mj);
                        }
                        wj = (float)(sg * (double)dtf * W);
                    }
                    wq[lb * 8 + j] = wj;
                }
                const double dtn = optimal_step_size_ni(dt, ratio);
                c.dt[lb] = dtn; c.dtf[lb] = (float)dtn;
                int dn = fin;
                if (!dn) {
                    const double tn = c.rk_t1[lb];
                    if ((long long)ns >= cfg.max_steps) { c.st[lb] = PHX_ERR_MAX_STEPS; dn = 2; }
                    else if (!(tn + dtn > tn)) { c.st[lb] = PHX_ERR_DT_UNDERFLOW; dn = 2; }
                }
                c.fin[lb] = dn;   // 0: continue, 1: reached t_{i-1}, 2: failed
            }
            __syncthreads();
            // the ring of a tile turns (k_7 -> k_1 without a copy) when every trajectory of it either continues with an
            // accepted step or is out of the interval after this step
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
            // The visit of the step that ends the solve goes to the tail kernel when nothing of the group's partial is
            // written yet and every trajectory of the group is either out already or reaches t_0 with this accepted step
            // (the benchmark's and training's case: one step per solve).  The decision is the same in all G workgroups
            // of the group (it reads controller values only); every other case takes the visit here, as before.
            if (may_defer && want_grads && iv == 1 && gfirst) {
                bool ok = !x.aborted;
                for (int lb = tid; lb < Bt; lb += blockDim.x) ok = ok && (c.done[lb] || (c.accept[lb] && c.fin[lb] == 1));
                ok = __all(ok) != 0;
                if (lane == 0) c.misc[4 + wv] = ok ? 1 : 0;   // (count_active's words: free between its calls)
                __syncthreads();
                for (int k = 0; k < d.NW; ++k) ok = ok && c.misc[4 + k] != 0;
                deferred = ok;
            }
            if (deferred) {
                if (gt == 0) {
                    for (int lb = tid; lb < Bt; lb += blockDim.x) {
                        float *rec = dth + (long long)lb * TR_N;
                        for (int j = 0; j < 7; ++j) rec[TR_W + j] = wq[lb * 8 + j];
                        rec[TR_DT] = c.dtp[lb];
                        rec[TR_SG] = c.sgn[lb];
                        const InterpX ix = make_interp_x(xfin[lb]);
                        rec[TR_X] = ix.x1; rec[TR_X + 1] = ix.x2; rec[TR_X + 2] = ix.x3; rec[TR_X + 3] = ix.x4;
                        rec[TR_ADV] = (!c.done[lb] && c.accept[lb]) ? 1.0f : 0.f;
                        rec[TR_ADV + 1] = 0.f; rec[TR_ADV + 2] = 0.f;
                    }
                    for (int i = tid; i < ntg; i += blockDim.x) reinterpret_cast<int *>(dth + (long long)Bt * TR_N)[i] = kbs[i];
                }
                tm.mark(10);
            } else
                quad_accept(iv);
            __syncthreads();
            if (tid < ntg && rotf[tid]) kbs[tid] = ring(kbs[tid], 6);
            if (tid < Bt && !c.done[tid] && c.fin[tid]) {
                c.done[tid] = 1;
                for (int j = 0; j < 8; ++j) wq[tid * 8 + j] = 0.f;
            }
            active = count_active();
        }
    }

    // ---- results (a deferred group's adj_y0 comes out of the tail kernel's accept pass)
    __syncthreads();
    if (want_grads && gt == 0 && tid == 0) xs.hdr[XH_DEFER + grp] = deferred ? 1u : 0u;
    for (int s = 0; s < d.TPW && !deferred; ++s) {
        const int ttl = wtile + s;
        if (ttl >= ntg) continue;
        const int b = grp * Bt + ttl * 16 + li;
        for (int bl = b_lo; bl < b_hi; ++bl) {
            float a0[8];
            load8(tptr(C_A0, ttl, bl), a0);
            row_store8(adj_y0, (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B, a0);
        }
    }
    // a group that never stepped (every trajectory failed before its first step) still owes its partial: every wave
    // clears the slots it would have written (quad_accept's ownership: half blocks wave, wave + NW, ...)
    if (want_grads && gfirst && !deferred) {
        for (int hb = wv; hb < 2 * nbl; hb += d.NW) {
            const int bl = hb >> 1, s2 = hb & 1;
            float4 *pn = reinterpret_cast<float4 *>(dth) + (long long)(blk0 + bl) * (F4 * 2 * 64) + lane;
            for (int mf = 0; mf < F4; ++mf) pn[(mf * 2 + s2) * 64] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (li == 0)
                for (int j = 0; j < 4; ++j) {
                    const int gene = (blk0 + bl) * 32 + gmap(lq, 4 * s2 + j);
                    if (gene < N) dth[og + gene] = 0.f;
                }
        }
        if (gt == 0 && wv == 0)
            for (int h = lane; h < H; h += 64) { dth[obs + h] = 0.f; dth[obp + h] = 0.f; }
    }
    tm.mark(0);
    if (tm.on) {
        for (int i = 0; i < 16; ++i) w.prof[(long long)blockIdx.x * 16 + i] = tm.acc[i];
        w.prof[(long long)blockIdx.x * 16 + 7] = (unsigned long long)clock64() - clk0;   // slot 7 is unused: shader cycles
    }
    if (gt == 0)
        for (int lb = tid; lb < Bt; lb += blockDim.x) {
            const int b = grp * Bt + lb;
            if (b < B) {
                status[b] = x.aborted ? (int)PHX_ERR_SYNC_TIMEOUT : c.st[lb];
                nfe_out[b] = c.nfe[lb];
                nsteps_out[b] = c.nsteps[lb];
            }
        }
    xset_end(xs, grp, gt, G);
}

}  // namespace
