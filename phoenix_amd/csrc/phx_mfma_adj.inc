// phx_mfma_adj.inc -- v1 backward pass of odeint_adjoint (MFMA, LDS-resident weights, group-local exchange).
// Algorithm and reference citations: see phx_adjoint.inc (v0) -- this file is the fast implementation of the
// same reverse-time augmented solve (adjoint.py:32-162) with the parameter gradient as a quadrature.
//
// Six contractions per augmented evaluation, all v_mfma_f32_16x16x4_f32 (layouts in phx_mfma_common.inc):
//   P1 u  = Ws . a        P2 v  = Wp . l        P3 dz = WaT . q          (contract genes; A = LDS form R)
//   P4 j  = Wa . z        P5 a~ = Ws^T . du     P6 l~ = Wp^T . dv        (contract hidden; A = LDS form C)
// and three per accepted step and stage for the quadrature (contract trajectories):
//   dWs += (w du)^T a     dWp += (w dv)^T l     dWaT += (w z)^T q        (A = stored hidden rows, B = stage tiles:
//                                                                          both read in natural layout and transposed
//                                                                          in registers, xpose4 in phx_mfma_common.inc)
namespace {

// private state vectors of the adjoint (tile-native scratch)
enum { A_Y0 = 0, A_A0 = 1, A_YS = 2, A_AS = 9, A_KY = 16, A_KA = 23, A_SG = 30, A_PJ = 37, A_PA = 38, A_PL = 39 };
constexpr int NVEC_ADJ = 37;
constexpr int NVEC_ADJ_CH = 40;   // + partial j, a~, l~ carried across hidden chunks

struct CtlA {
    Ctl c;
    double *xfin;   // [Bt]
    float *wq;      // [Bt][8]
};
__host__ __device__ inline size_t ctla_bytes(int Bt) { return ctl_bytes(Bt) + (size_t)Bt * 8 + (size_t)Bt * 8 * 4; }

__device__ __forceinline__ void act_grad_fast(float y, float &da, float &dl)
{
    const float s = y - 0.5f;
    const float d = 1.0f + fabsf(s);
    const float rd = fast_rcp(d);
    da = rd * rd;
    dl = (s < 0.0f) ? rd : fast_rcp((1.0f + s) * (1.0f + 2.0f * s));
}

// CH: hidden layer in d.HC chunks of d.Hc rows (see k1_solve_fwd); all six contractions are sums over hidden rows
// or produce per-row outputs, so every chunk is an independent slice of the same evaluation.
}  // namespace
namespace phxk {   // external linkage: instantiated in phx_v1.hip, launched from phx_engine.hip
template <int HT, int MAXT, bool CH>
__global__ __launch_bounds__(MAXT) void k1_solve_adj(Net net, D1 d, W1 w, SolveCfg cfg, const double *__restrict__ t,
                                                     const float *__restrict__ y_saved,
                                                     const float *__restrict__ grad_y, float *adj_y0, int *status,
                                                     int *nfe_out, int *nsteps_out, int want_grads, long long PP)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, H = d.H, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G;
    const int HC = CH ? d.HC : 1, Hc = CH ? d.Hc : H;
    const int BLKF = blk_floats_ch(HT, Hc);   // slots are float4-copyable packed images (k1_pack_images)
    const int RGOFF = BLKF - 32;
    const bool shared = cfg.control == PHX_CTRL_SHARED;
    constexpr int F4 = 4 * HT, F2 = 2 * HT;
    const int F4T = F4 * HC;
    float *ctlbase = lds + (long long)d.NB * BLKF;
    Ctl c = carve_ctl(ctlbase, Bt);
    double *xfin = reinterpret_cast<double *>(reinterpret_cast<char *>(ctlbase) + ctl_bytes(Bt));
    float *wq = reinterpret_cast<float *>(xfin + Bt);
    const int RH = ntg * F4T * 4;  // hidden rows (u, v, dz_u, dz_p per chunk) of one exchange; norm rows follow
    const int R = RH + ntg;
    Xchg x{w.part + (long long)grp * G * R * 64, w.zbuf + (long long)grp * R * 64, (long long)d.TG * R * 64,
           w.abort_flag, 0u, G, gt, R, false};
    SegTimer tm;
    tm.start(w.prof != nullptr, c.tacc);

    stage_images(w.wimg, lds, blk0, nbl, 0, HC, BLKF);
    int resident = 0;
    auto hc_of = [&](int ch) -> int { return min(Hc, H - ch * Hc); };
    auto ensure = [&](int ch, int seg) {
        if (!CH || resident == ch) return;
        tm.mark(seg);
        __syncthreads();
        stage_images(w.wimg, lds, blk0, nbl, ch, HC, BLKF);
        __syncthreads();
        resident = ch;
        tm.mark(15);   // weight re-staging of a hidden chunk
    };
    auto chunk_at = [&](int r0, int ci) -> int { return ci == 0 ? r0 : (ci <= r0 ? ci - 1 : ci); };

    const int offR = li * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = 4 * lq * LROW + gmapC(li, 0);
    offC[1] = 4 * lq * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * d.nvec * tiles_wg * 512;
    auto tbase = [&](int v, int ttl, int bl) -> float * {
        return wgbase + ((long long)v * tiles_wg + (ttl * d.NB + bl)) * 512;
    };
    auto tptr = [&](int v, int ttl, int bl) -> float * { return tbase(v, ttl, bl) + lane * 8; };
    // reduced hidden rows of stage slot `slot`: [slot][grp][R][64] granules
    auto zrowf = [&](int slot, int ttl, int fidx, int r) -> u64 * {   // fidx in [0, F4T): chunk * F4 + f4
        return x.zbuf + (long long)slot * x.zslot + ((long long)(ttl * F4T + fidx) * 4 + r) * 64;
    };
    auto zrow = [&](int slot, int ttl, int ch, int f4, int r) -> u64 * { return zrowf(slot, ttl, ch * F4 + f4, r); };
    float *dth = w.dtheta + (long long)(grp * d.NW + wv) * PP;   // this wave's parameter-gradient partial
    const long long oWs = 0, oWp = (long long)H * N, oWa = 2LL * H * N, og = 4LL * H * N, obs = og + N, obp = obs + H;

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
        c.accept[lb] = 0; c.fin[lb] = 0; c.out_lo[lb] = 0;   // out_lo: steps of the current interval
        for (int j = 0; j < 8; ++j) wq[lb * 8 + j] = 0.f;
    }
    // ---- terminal state (adjoint.py:86-87)
    for (int s = 0; s < d.TPW; ++s) {
        const int ttl = wv * d.TPW + s;
        if (ttl >= ntg) continue;
        const int b = grp * Bt + ttl * 16 + li;
        for (int bl = 0; bl < nbl; ++bl) {
            float x[8], a[8];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
            const long long ro = (long long)(T - 1) * d.BN + (long long)b * N;
            row_load8(y_saved, ro, g0, N, b < B, 0.5f, x);
            row_load8(grad_y, ro, g0, N, b < B, 0.f, a);
            store8(tptr(A_Y0, ttl, bl), x);
            store8(tptr(A_A0, ttl, bl), a);
        }
    }
    __syncthreads();
    tm.mark(6);

    auto count_active = [&]() -> int {
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int lb = 0; lb < Bt; ++lb) n += c.done[lb] ? 0 : 1;
            c.misc[0] = n;
        }
        __syncthreads();
        return c.misc[0];
    };
    const bool stepped = cfg.method != PHX_DOPRI5 && cfg.step > 0.0;   // options["step_size"]: see k1_solve_adj2
    auto dt_rev = [&](int lb, int iv) -> float {   // reversed pair (-t_i, -t_{i-1}) of the fixed grid
        if (stepped) return c.dtf[lb];             // ... or the running step of the interval's own grid
        const int b = grp * Bt + lb;
        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : min(b, B - 1));
        const double sg = (double)c.sgn[lb];
        const double u0 = -sg * tb[iv], u1 = -sg * tb[iv - 1];
        return cfg.t_is_f32 ? ((float)u1 - (float)u0) : (float)(u1 - u0);
    };

    // Reduce-scatter of rows [row0,row0+nrows) into z slot `slot` (see k1_solve_fwd); `comp(u)` names a second
    // row to be reduced alongside (dv = dz_p * p needs the matching v row), or -1.
    auto reduce_rows = [&](int slot, int row0, int nrows, auto comp, auto post) {
        if (G <= 16) {
            // few members: one wave per row, one batch of loads per row (see k1_solve_fwd); the barrier at the end
            // restores the workgroup-wide "my rows are complete" guarantee the FSAL copy below relies on
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
                st_gran(x.zbuf + (long long)slot * x.zslot + (long long)row * 64, lane, post(u, tot, ctot), x.tag);
            }
            __syncthreads();
            return;
        }
        if (G > 128) {
            // very wide groups (C5: 230 members, 18 owned rows per evaluation): two owned rows per pass, 32 member loads
            // in flight per wave -- half the dependent round trips.  (Narrower groups measured slower this way: the
            // heavier polling costs more than the round trips it saves.)
            for (int u = gt; u < nrows; u += 2 * G) {
                const bool hasB = u + G < nrows;
                const int uB = hasB ? u + G : u;
                const int rowA = row0 + u, rowB = row0 + uB;
                const int crowA = comp(u), crowB = hasB ? comp(uB) : -1;
                float sA = 0.f, sB = 0.f, cA = 0.f, cB = 0.f;
                for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                    const u64 *rows[32];
                    int nv = 0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int gg = g2 + k * d.NW;
                        const long long mb = (long long)min(gg, G - 1) * R;
                        rows[k] = x.part + (mb + rowA) * 64;
                        rows[16 + k] = x.part + (mb + rowB) * 64;
                        nv += (gg < G) ? 1 : 0;
                    }
                    float v[32];
                    wait_rows<32>(x, rows, 32, lane, v);   // clamped members are real rows: every entry is valid
#pragma unroll
                    for (int k = 0; k < 16; ++k) { sA += (k < nv) ? v[k] : 0.f; sB += (k < nv) ? v[16 + k] : 0.f; }
                    if (crowA >= 0 || crowB >= 0) {
#pragma unroll
                        for (int k = 0; k < 16; ++k) {
                            const int gg = g2 + k * d.NW;
                            const long long mb = (long long)min(gg, G - 1) * R;
                            rows[k] = x.part + (mb + (crowA >= 0 ? crowA : rowA)) * 64;
                            rows[16 + k] = x.part + (mb + (crowB >= 0 ? crowB : rowB)) * 64;
                        }
                        wait_rows<32>(x, rows, 32, lane, v);
#pragma unroll
                        for (int k = 0; k < 16; ++k) { cA += (k < nv) ? v[k] : 0.f; cB += (k < nv) ? v[16 + k] : 0.f; }
                    }
                }
                // combine through LDS: [row A | companion A | row B | companion B][wave]
                c.wred[(0 * 4 + wv) * 64 + lane] = sA;
                c.wred[(1 * 4 + wv) * 64 + lane] = cA;
                c.wred[(2 * 4 + wv) * 64 + lane] = sB;
                c.wred[(3 * 4 + wv) * 64 + lane] = cB;
                __syncthreads();
                if (wv < 2 && (wv == 0 || hasB)) {   // wave 0 publishes row A, wave 1 row B
                    float tot = 0.f, ctot = 0.f;
                    for (int k = 0; k < d.NW; ++k) {
                        tot += c.wred[((2 * wv) * 4 + k) * 64 + lane];
                        ctot += c.wred[((2 * wv + 1) * 4 + k) * 64 + lane];
                    }
                    const int uu = wv == 0 ? u : uB;
                    st_gran(x.zbuf + (long long)slot * x.zslot + (long long)(row0 + uu) * 64, lane, post(uu, tot, ctot), x.tag);
                }
                __syncthreads();   // the combine buffer is reused by the next pair
            }
            __syncthreads();       // workgroup-wide "my rows are complete" point also when the workgroup owns none
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
                st_gran(x.zbuf + (long long)slot * x.zslot + (long long)row * 64, lane, post(u, tot, ctot), x.tag);
            }
            wbuf ^= 1;
        }
        __syncthreads();   // the combine buffers are free again; also the workgroup-wide "my rows are complete" point
    };

    // One augmented evaluation.  smode 0: (Y0,A0)  1: +h0*K0  2: dopri5 stage st  3: fixed-grid stage st
    // slot: where stage inputs / K / SG / hidden buffers of this evaluation are kept
    // rmode 0 none, 1: d0,d1 of both blocks, 2: d2 of both blocks, 3: error ratio of both blocks
    auto eval_aug = [&](int smode, int st, int iv, int slot, int rmode) {
        tm.mark(0);
        x.tag += 1u;
        // ---------------- P1'
        const int r0p1 = resident;
        for (int ci = 0; ci < HC; ++ci) {
        const int ch = CH ? chunk_at(r0p1, ci) : 0;
        ensure(ch, 1);
        const int hc = CH ? hc_of(ch) : H;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const int lb = ttl * 16 + li;
            const int b = grp * Bt + lb;
            f32x4 acc[F4];
#pragma unroll
            for (int f = 0; f < F4; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float dtl = 0.f;
            if (smode == 1) dtl = c.h0f[lb];
            else if (smode == 2) dtl = c.dtf[lb];
            else if (smode == 3) dtl = dt_rev(lb, iv);
            // dopri5 stages: the state tiles of gene block bl+1 are requested before the MFMA chain of block bl
            // (P1' is not the register-critical phase of this kernel), so only the first block exposes its latency
            const bool pf = (smode == 2) && !(CH && ci > 0);
            float pys[8], pas[8], pky[6][8], pka[6][8];
            auto request = [&](int bl_) {
                load8(tptr(A_Y0, ttl, bl_), pys);
                load8(tptr(A_A0, ttl, bl_), pas);
#pragma unroll
                for (int kk = 0; kk < 6; ++kk)
                    if (kk < st) {   // k2 has a structurally zero weight in the last row of the tableau
                        if (st == 6 && kk == 1) { zero8(pky[kk]); zero8(pka[kk]); }
                        else { load8(tptr(A_KY + kk, ttl, bl_), pky[kk]); load8(tptr(A_KA + kk, ttl, bl_), pka[kk]); }
                    }
            };
            if (pf) request(0);
            for (int bl = 0; bl < nbl; ++bl) {
                float ys[8], as[8];
                if (pf) {
                    float accy[8], acca[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { accy[j] = 0.f; acca[j] = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) {
                            const float cf = DP_BETA[st - 1][kk] * dtl;
#pragma unroll
                            for (int j = 0; j < 8; ++j) { accy[j] += pky[kk][j] * cf; acca[j] += pka[kk][j] * cf; }
                        }
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ys[j] = pys[j] + accy[j]; as[j] = pas[j] + acca[j]; }
                    // never under a condition (the last block re-requests itself): a conditional request makes the compiler
                    // merge register versions of the prefetch buffers with copies, which wait for the loads at once
                    request(min(bl + 1, nbl - 1));
                } else if (CH && ci > 0) {   // stage inputs were formed and stored by the first chunk's pass
                    load8(tptr(A_YS + slot, ttl, bl), ys);
                    load8(tptr(A_AS + slot, ttl, bl), as);
                } else {
                    load8(tptr(A_Y0, ttl, bl), ys);
                    load8(tptr(A_A0, ttl, bl), as);
                }
                if (pf || (CH && ci > 0)) {
                } else if (smode == 1) {
                    float ky[8], ka[8];
                    load8(tptr(A_KY, ttl, bl), ky);
                    load8(tptr(A_KA, ttl, bl), ka);
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ys[j] = ys[j] + dtl * ky[j]; as[j] = as[j] + dtl * ka[j]; }
                } else if (smode == 2) {
                    // all stage tiles of the y AND the a block are requested back to back: one memory round trip per
                    // gene block (P1' is not the register-critical phase of this kernel, the quadrature is)
                    float kqy[6][8], kqa[6][8];
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) load8(tptr(A_KY + kk, ttl, bl), kqy[kk]);
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) load8(tptr(A_KA + kk, ttl, bl), kqa[kk]);
                    float accy[8], acca[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { accy[j] = 0.f; acca[j] = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) {
                            const float cf = DP_BETA[st - 1][kk] * dtl;
#pragma unroll
                            for (int j = 0; j < 8; ++j) { accy[j] += kqy[kk][j] * cf; acca[j] += kqa[kk][j] * cf; }
                        }
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ys[j] = ys[j] + accy[j]; as[j] = as[j] + acca[j]; }
                } else if (smode == 3 && st > 0) {
                    const float third = (float)(1.0 / 3.0);
                    float y0k[8], y1k[8], y2k[8], a0k[8], a1k[8], a2k[8];
                    load8(tptr(A_KY, ttl, bl), y0k);
                    load8(tptr(A_KA, ttl, bl), a0k);
                    if (cfg.method == PHX_MIDPOINT) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            ys[j] = ys[j] + y0k[j] * (0.5f * dtl);
                            as[j] = as[j] + a0k[j] * (0.5f * dtl);
                        }
                    } else if (st == 1) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            ys[j] = ys[j] + (dtl * y0k[j]) * third;
                            as[j] = as[j] + (dtl * a0k[j]) * third;
                        }
                    } else if (st == 2) {
                        load8(tptr(A_KY + 1, ttl, bl), y1k);
                        load8(tptr(A_KA + 1, ttl, bl), a1k);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            ys[j] = ys[j] + dtl * (y1k[j] - y0k[j] * third);
                            as[j] = as[j] + dtl * (a1k[j] - a0k[j] * third);
                        }
                    } else {
                        load8(tptr(A_KY + 1, ttl, bl), y1k);
                        load8(tptr(A_KA + 1, ttl, bl), a1k);
                        load8(tptr(A_KY + 2, ttl, bl), y2k);
                        load8(tptr(A_KA + 2, ttl, bl), a2k);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            ys[j] = ys[j] + dtl * ((y0k[j] - y1k[j]) + y2k[j]);
                            as[j] = as[j] + dtl * ((a0k[j] - a1k[j]) + a2k[j]);
                        }
                    }
                }
                if (!(CH && ci > 0)) {
                    store8(tptr(A_YS + slot, ttl, bl), ys);
                    store8(tptr(A_AS + slot, ttl, bl), as);
                }
                const float *Wb = lds + (long long)bl * BLKF;
                const float *rg = Wb + RGOFF;
                float av[8], lv[8], qv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                    const bool ok = (b < B) && (gene < N);
                    float a = 0.f, l = 0.f;
                    if (ok) act_pair_fast(ys[j], a, l);
                    av[j] = a; lv[j] = l;
                    qv[j] = ok ? as[j] * rg[gmap(lq, j)] : 0.f;
                }
                const float *Wr = Wb + offR;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        acc[f] = mfma4(Wr[f * 16 * LROW + j], av[j], acc[f]);
                        acc[HT + f] = mfma4(Wr[(hc + f * 16) * LROW + j], lv[j], acc[HT + f]);
                    }
#pragma unroll
                    for (int f = 0; f < F2; ++f)
                        acc[F2 + f] = mfma4(Wr[((f < HT ? 2 * hc + 16 * f : 3 * hc + 16 * (f - HT))) * LROW + j], qv[j], acc[F2 + f]);
                }
            }
            u64 *pp = x.part + ((long long)gt * R + ((long long)ttl * F4T + ch * F4) * 4) * 64;
#pragma unroll
            for (int f = 0; f < F4; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) st_gran(pp + ((long long)f * 4 + r) * 64, lane, acc[f][r], x.tag);
        }
        }
        tm.mark(1);
        // ---------------- reduce-scatter (z, du, dv)
        reduce_rows(slot, 0, RH,
                    [&](int u) -> int {   // dv rows (dz_p part) also need their v row
                        const int f4 = (u >> 2) % F4;
                        return (f4 >= 3 * HT) ? u - F2 * 4 : -1;
                    },
                    [&](int u, float tot, float totv) -> float {
                        const int r = u & 3, f4t = (u >> 2) % F4T, ch = f4t / F4, f4 = f4t % F4;
                        const int rowl = 16 * (f4 % HT) + 4 * lq + r;
                        if (rowl >= (CH ? hc_of(ch) : H)) return 0.f;
                        const int row = ch * Hc + rowl;
                        if (f4 < HT) return tot + net.bs[row];
                        if (f4 < F2) return expf(tot + net.bp[row]);
                        if (f4 < 3 * HT) return tot;                    // du
                        return tot * expf(totv + net.bp[row]);          // dv = dz_p * p
                    });
        // FSAL of the hidden rows (stage 7 of the previous step -> stage 1 of this one).  Done here, by the
        // owner of a tile's first row, because completing that row proves that every member's wave of this
        // tile has left the previous step's quadrature pass (the only reader of slot 0).
        if (want_grads && smode == 2 && st == 1) {
            for (int u = gt; u < RH; u += G) {
                if (u % (F4T * 4) != 0) continue;
                const int ttl = u / (F4T * 4);
                const int lbc = ttl * 16 + li;
                const bool cp = c.accept[lbc] && c.fin[lbc] == 0;
                for (int k = wv; k < F4T * 4; k += d.NW) {
                    const float v = ld_gran_val(zrowf(6, ttl, k >> 2, k & 3) + lane);
                    if (cp) st_gran(zrowf(0, ttl, k >> 2, k & 3), lane, v, 0u);
                }
            }
        }
        tm.mark(3);
        // ---------------- P2'
        const int r0p2 = resident;
        for (int ci = 0; ci < HC; ++ci) {
        const int ch = CH ? chunk_at(r0p2, ci) : 0;
        ensure(ch, 5);
        const int hc = CH ? hc_of(ch) : H;
        const bool firstc = ci == 0, lastc = ci == HC - 1;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const int lb = ttl * 16 + li;
            const int b = grp * Bt + lb;
            float zr[F4][4];
#pragma unroll
            for (int f4 = 0; f4 < F4; f4 += 4) {   // F4 = 4 HT is a multiple of four: 16 rows per batch
                const u64 *rows[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) rows[k] = zrow(slot, ttl, ch, f4 + (k >> 2), k & 3);
                float v[16];
                wait_rows<16>(x, rows, 16, lane, v);
#pragma unroll
                for (int k = 0; k < 16; ++k) zr[f4 + (k >> 2)][k & 3] = v[k];
            }
            if (s == 0 && firstc) tm.mark(4);
            const float sg = c.sgn[lb];
            float dtl = 0.f;
            if (smode == 2) dtl = c.dtf[lb];
            float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
            for (int bl = 0; bl < nbl; ++bl) {
                const float *Wb = lds + (long long)bl * BLKF;
                float ys[8], as[8], y0v[8], a0v[8], ky0[8], ka0[8], pj[8], pa[8], pl[8];
                if (CH && !firstc) {
                    load8(tptr(A_PJ, ttl, bl), pj);
                    load8(tptr(A_PA, ttl, bl), pa);
                    load8(tptr(A_PL, ttl, bl), pl);
                }
                if (lastc) {
                    load8(tptr(A_YS + slot, ttl, bl), ys);
                    load8(tptr(A_AS + slot, ttl, bl), as);
                    if (rmode >= 2) { load8(tptr(A_Y0, ttl, bl), y0v); load8(tptr(A_A0, ttl, bl), a0v); }
                    if (rmode == 2) { load8(tptr(A_KY, ttl, bl), ky0); load8(tptr(A_KA, ttl, bl), ka0); }
                }
                float jv[8], dap[8], dlp[8];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    f32x4 aj = (f32x4){0.f, 0.f, 0.f, 0.f}, aa = aj, al = aj;
                    const float *Wc = Wb + offC[s2];
#pragma unroll
                    for (int f2 = 0; f2 < F2; ++f2) {
                        const int rb = (f2 < HT) ? 2 * hc + 16 * f2 : 3 * hc + 16 * (f2 - HT);
#pragma unroll
                        for (int r = 0; r < 4; ++r) aj = mfma4(Wc[(rb + r) * LROW], zr[f2][r], aj);
                    }
#pragma unroll
                    for (int f = 0; f < HT; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            aa = mfma4(Wc[(16 * f + r) * LROW], zr[F2 + f][r], aa);
                            al = mfma4(Wc[(hc + 16 * f + r) * LROW], zr[3 * HT + f][r], al);
                        }
#pragma unroll
                    for (int r = 0; r < 4; ++r) { jv[4 * s2 + r] = aj[r]; dap[4 * s2 + r] = aa[r]; dlp[4 * s2 + r] = al[r]; }
                }
                if (CH) {   // j, a~, l~ are sums over the hidden chunks: partials travel through private tiles
                    if (!firstc) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) { jv[j] += pj[j]; dap[j] += pa[j]; dlp[j] += pl[j]; }
                    }
                    if (!lastc) {
                        store8(tptr(A_PJ, ttl, bl), jv);
                        store8(tptr(A_PA, ttl, bl), dap);
                        store8(tptr(A_PL, ttl, bl), dlp);
                        continue;
                    }
                }
                const float *rg = Wb + RGOFF;
                float ky[8], ka[8], sgv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float rr = rg[gmap(lq, j)];
                    const float dj = jv[j] - ys[j];
                    float da, dl;
                    act_grad_fast(ys[j], da, dl);
                    const float vjp = (dap[j] * da + dlp[j] * dl) - as[j] * rr;
                    ky[j] = -sg * (rr * dj);
                    ka[j] = sg * vjp;
                    sgv[j] = (rr > 0.f) ? as[j] * dj : 0.f;
                }
                store8(tptr(A_KY + slot, ttl, bl), ky);
                store8(tptr(A_KA + slot, ttl, bl), ka);
                if (want_grads) store8(tptr(A_SG + slot, ttl, bl), sgv);
                if (rmode != 0) {
                    float ey[8], ea[8];
                    if (rmode == 3) {
#pragma unroll
                        for (int part = 0; part < 2; ++part) {
                            float kq[6][8];
#pragma unroll
                            for (int kk = 0; kk < 6; ++kk) {   // DP_CERR[1] == 0: k2 is not read
                                if (kk == 1) zero8(kq[kk]);
                                else load8(tptr((part ? A_KA : A_KY) + kk, ttl, bl), kq[kk]);
                            }
                            float e8[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) e8[j] = 0.f;
#pragma unroll
                            for (int kk = 0; kk < 6; ++kk) {
                                const float cf = dtl * DP_CERR[kk];
#pragma unroll
                                for (int j = 0; j < 8; ++j) e8[j] += kq[kk][j] * cf;
                            }
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                if (part) ea[j] = e8[j];
                                else ey[j] = e8[j];
                            }
                        }
                        const float cf6 = dtl * DP_CERR[6];
#pragma unroll
                        for (int j = 0; j < 8; ++j) { ey[j] += ky[j] * cf6; ea[j] += ka[j] * cf6; }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                        if (!((b < B) && (gene < N))) continue;
                        if (rmode == 1) {
                            const float sy = cfg.atol + fabsf(ys[j]) * cfg.rtol, sa = cfg.atol + fabsf(as[j]) * cfg.rtol;
                            const float q0 = ys[j] / sy, q1 = as[j] / sa, q2 = ky[j] / sy, q3 = ka[j] / sa;
                            r0 += q0 * q0; r1 += q1 * q1; r2 += q2 * q2; r3 += q3 * q3;
                        } else if (rmode == 2) {
                            const float sy = cfg.atol + fabsf(y0v[j]) * cfg.rtol, sa = cfg.atol + fabsf(a0v[j]) * cfg.rtol;
                            const float q0 = (ky[j] - ky0[j]) / sy, q1 = (ka[j] - ka0[j]) / sa;
                            r0 += q0 * q0; r1 += q1 * q1;
                        } else {
                            const float ty = cfg.atol + cfg.rtol * fmaxf(fabsf(y0v[j]), fabsf(ys[j]));
                            const float ta = cfg.atol + cfg.rtol * fmaxf(fabsf(a0v[j]), fabsf(as[j]));
                            const float q0 = ey[j] / ty, q1 = ea[j] / ta;
                            r0 += q0 * q0; r1 += q1 * q1;
                        }
                    }
                }
            }
            if (rmode != 0 && lastc) {
                r0 = sum_over_q(r0); r1 = sum_over_q(r1); r2 = sum_over_q(r2); r3 = sum_over_q(r3);
                st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane,
                        lq == 0 ? r0 : (lq == 1 ? r1 : (lq == 2 ? r2 : r3)), x.tag + 1u);
            }
        }
        }
        if (rmode != 0) x.tag += 1u;
        tm.mark(5);
    };

    // ---- mixed Linf/RMS norm over the [y, a] blocks (misc.py:14-24): slot pairs (0,1) and (2,3)
    auto norms = [&](float *out2) {
        reduce_rows(0, RH, ntg, [&](int) -> int { return -1; }, [&](int, float tot, float) -> float { return tot; });
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
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
    };

    // ---- parameter-gradient quadrature of the stages [0, S) with the weights wq (zero => skipped).
    // Loop order: [pass A | pass B] x chunk of QB gene blocks x stage.  Per stage the hidden rows (the MFMA A
    // operands, identical for every gene block) are gathered ONCE and all QB blocks' state tiles are requested
    // together, so each stage exposes one memory latency; the QB blocks' accumulators live in AGPRs.
    // pass A: dWs += (w du)^T a, dWp += (w dv)^T l, dg += w sg   (needs y, sg, du, dv)
    // pass B: dWaT += (w z)^T q                                  (needs adj, z)
    // First touch of a wave's partial uses plain stores (no memset, no read); later steps read-add-store.
    bool gfirst = true;
    constexpr int QB = (HT == 3) ? 2 : 1;   // 3 spilled 125 registers and lost 2 % overall
    auto phaseG = [&](int S) {
        tm.mark(0);
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            float wany = 0.f;
            for (int j = 0; j < S; ++j) wany += fabsf(wq[(ttl * 16 + li) * 8 + j]);
            const bool wr_first = gfirst && s == 0;
            if (!__any(wany != 0.f) && !wr_first) continue;
            const int zl = (li >> 2) * 16 + 4 * lq;                         // lane part of the hidden-row gathers
            for (int bl0 = 0; bl0 < nbl; bl0 += QB)
            for (int ch = 0; ch < HC; ++ch) {
                const int hc = CH ? hc_of(ch) : H;
                const int hb = ch * Hc;
                // ---------------- pass A
                {
                    f32x4 gs_[QB][HT][2], gp_[QB][HT][2];
                    float dgacc[QB][2];
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        dgacc[qb][0] = 0.f; dgacc[qb][1] = 0.f;
#pragma unroll
                        for (int f = 0; f < HT; ++f)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) { gs_[qb][f][s2] = (f32x4){0.f, 0.f, 0.f, 0.f}; gp_[qb][f][s2] = gs_[qb][f][s2]; }
                    }
                    for (int sidx = 0; sidx < S; ++sidx) {
                        const float wl = wq[(ttl * 16 + li) * 8 + sidx];
                        if (!__any(wl != 0.f)) continue;
                        float w4[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) w4[r] = wq[(ttl * 16 + 4 * lq + r) * 8 + sidx];
                        // every operand is read in its natural (coalesced) layout and transposed in registers
                        float hd[F2][4], yr[QB][2][4], gr[QB][2][4];
                        float hnat[F2][4], ynat[QB][8], gnat[QB][8];
#pragma unroll
                        for (int f = 0; f < F2; ++f)
#pragma unroll
                            for (int r = 0; r < 4; ++r) hnat[f][r] = ld_gran_val(zrow(sidx, ttl, ch, F2 + f, r) + lane);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb) {
                            const int bl = min(bl0 + qb, nbl - 1);
                            load8(tptr(A_YS + sidx, ttl, bl), ynat[qb]);
                            load8(tptr(A_SG + sidx, ttl, bl), gnat[qb]);
                        }
#pragma unroll
                        for (int f = 0; f < F2; ++f) xpose4(hnat[f], hd[f], lane);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) {
                                xpose4(&ynat[qb][4 * s2], yr[qb][s2], lane);
                                xpose4(&gnat[qb][4 * s2], gr[qb][s2], lane);
                            }
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb) {
                            if (bl0 + qb >= nbl) continue;
                            const int gene0 = (blk0 + bl0 + qb) * 32;
                            float av[2][4], lv[2][4];
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) {
                                const bool gok = (gene0 + gmapC(li, s2)) < N;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const bool ok = gok && (grp * Bt + ttl * 16 + 4 * lq + r) < B;
                                    float a = 0.f, l = 0.f;
                                    if (ok) act_pair_fast(yr[qb][s2][r], a, l);
                                    av[s2][r] = a; lv[s2][r] = l;
                                    if (ok) dgacc[qb][s2] += w4[r] * gr[qb][s2][r];
                                }
                            }
#pragma unroll
                            for (int f = 0; f < HT; ++f)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float du = w4[r] * hd[f][r], dv = w4[r] * hd[HT + f][r];
#pragma unroll
                                    for (int s2 = 0; s2 < 2; ++s2) {
                                        gs_[qb][f][s2] = mfma4(du, av[s2][r], gs_[qb][f][s2]);
                                        gp_[qb][f][s2] = mfma4(dv, lv[s2][r], gp_[qb][f][s2]);
                                    }
                                }
                        }
                    }
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        if (bl0 + qb >= nbl) continue;
                        const int gene0 = (blk0 + bl0 + qb) * 32;
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) {
                            const int gene = gene0 + gmapC(li, s2);
                            // accumulators are quad-transposed so that a lane owns four consecutive genes of ONE row:
                            // 16-byte accesses, whole 128-byte lines per row segment
                            const int gene4 = gene0 + gmapC(li & ~3, s2), rowq = 4 * lq + (li & 3);
#pragma unroll
                            for (int f = 0; f < HT; ++f) {
                                float a4[4], b4[4], t0[4], t1[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) { a4[r] = gs_[qb][f][s2][r]; b4[r] = gp_[qb][f][s2][r]; }
                                quad_transpose(a4, t0, lane);
                                quad_transpose(b4, t1, lane);
                                if (16 * f + rowq < hc && gene4 < N) {
                                    add_store4(dth + oWs + (long long)(hb + 16 * f + rowq) * N + gene4, t0, gene4, N, wr_first);
                                    add_store4(dth + oWp + (long long)(hb + 16 * f + rowq) * N + gene4, t1, gene4, N, wr_first);
                                }
                            }
                            float dg = dgacc[qb][s2];
                            dg += __shfl_xor(dg, 16, 64);
                            dg += __shfl_xor(dg, 32, 64);
                            if (lq == 0 && gene < N && ch == 0) dth[og + gene] = (wr_first ? 0.f : dth[og + gene]) + dg;
                        }
                    }
                }
                // ---------------- pass B
                {
                    f32x4 ga_[QB][F2][2];
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                        for (int f = 0; f < F2; ++f)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) ga_[qb][f][s2] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    for (int sidx = 0; sidx < S; ++sidx) {
                        const float wl = wq[(ttl * 16 + li) * 8 + sidx];
                        if (!__any(wl != 0.f)) continue;
                        float w4[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) w4[r] = wq[(ttl * 16 + 4 * lq + r) * 8 + sidx];
                        float hz[F2][4], ar[QB][2][4];
                        float hnat[F2][4], anat[QB][8];
#pragma unroll
                        for (int f = 0; f < F2; ++f)
#pragma unroll
                            for (int r = 0; r < 4; ++r) hnat[f][r] = ld_gran_val(zrow(sidx, ttl, ch, f, r) + lane);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb) load8(tptr(A_AS + sidx, ttl, min(bl0 + qb, nbl - 1)), anat[qb]);
#pragma unroll
                        for (int f = 0; f < F2; ++f) xpose4(hnat[f], hz[f], lane);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) xpose4(&anat[qb][4 * s2], ar[qb][s2], lane);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb) {
                            if (bl0 + qb >= nbl) continue;
                            const int gene0 = (blk0 + bl0 + qb) * 32;
                            const float *rg = lds + (long long)(bl0 + qb) * BLKF + RGOFF;
                            float qv[2][4];
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) {
                                const bool gok = (gene0 + gmapC(li, s2)) < N;
                                const float rr = rg[gmapC(li, s2)];
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const bool ok = gok && (grp * Bt + ttl * 16 + 4 * lq + r) < B;
                                    qv[s2][r] = ok ? ar[qb][s2][r] * rr : 0.f;
                                }
                            }
#pragma unroll
                            for (int f = 0; f < F2; ++f)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float zz = w4[r] * hz[f][r];
#pragma unroll
                                    for (int s2 = 0; s2 < 2; ++s2) ga_[qb][f][s2] = mfma4(zz, qv[s2][r], ga_[qb][f][s2]);
                                }
                        }
                    }
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        if (bl0 + qb >= nbl) continue;
                        const int gene0 = (blk0 + bl0 + qb) * 32;
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) {
                            const int gene4 = gene0 + gmapC(li & ~3, s2), rowq = 4 * lq + (li & 3);
#pragma unroll
                            for (int f = 0; f < HT; ++f) {
                                float a4[4], b4[4], t0[4], t1[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) { a4[r] = ga_[qb][f][s2][r]; b4[r] = ga_[qb][HT + f][s2][r]; }
                                quad_transpose(a4, t0, lane);
                                quad_transpose(b4, t1, lane);
                                if (16 * f + rowq < hc && gene4 < N) {
                                    add_store4(dth + oWa + (long long)(hb + 16 * f + rowq) * N + gene4, t0, gene4, N, wr_first);
                                    add_store4(dth + oWa + (long long)(H + hb + 16 * f + rowq) * N + gene4, t1, gene4, N, wr_first);
                                }
                            }
                        }
                    }
                }
            }
            // bias gradients: gene independent => only the first gene tile of the group accumulates them
            if (gt == 0)
            for (int ch = 0; ch < HC; ++ch) {
                const int hc = CH ? hc_of(ch) : H;
                for (int f = 0; f < HT; ++f) {
                    float sb = 0.f, sp = 0.f;
                    for (int sidx = 0; sidx < S; ++sidx) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float wr = wq[(ttl * 16 + 4 * lq + r) * 8 + sidx];
                            if (wr != 0.f) {
                                sb += wr * ld_gran_val(zrow(sidx, ttl, ch, F2 + f, li & 3) + zl + r);
                                sp += wr * ld_gran_val(zrow(sidx, ttl, ch, 3 * HT + f, li & 3) + zl + r);
                            }
                        }
                    }
                    sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
                    sp += __shfl_xor(sp, 16, 64); sp += __shfl_xor(sp, 32, 64);
                    const int hid = ch * Hc + 16 * f + li;
                    if (lq == 0 && (16 * f + li) < hc) {
                        dth[obs + hid] = (wr_first ? 0.f : dth[obs + hid]) + sb;
                        dth[obp + hid] = (wr_first ? 0.f : dth[obp + hid]) + sp;
                    }
                }
            }
        }
        gfirst = false;
        tm.mark(11);
    };

    float nv[2];
    for (int iv = T - 1; iv >= 1; --iv) {
        if (stepped) {
            // ------------------------------------------------------------ fixed grid with a step size (adjoint.py:137-154
            // calls odeint per interval): the interval's own grid anchored at its start, one set of quadrature weights per
            // step, the jump after the last one.  out_lo = steps of the grid, out_hi = steps taken, rk_t0 / rk_t1 = the
            // running step; a trajectory whose grid has ended is masked by `done` until the next interval.
            const int S = fixed_nstages(cfg.method);
            const bool tf32 = cfg.t_is_f32 != 0;
            __syncthreads();
            for (int lb = tid; lb < Bt; lb += blockDim.x) {
                const int b = grp * Bt + lb;
                c.dtf[lb] = 0.f;
                if (b >= B || c.st[lb] != PHX_OK) { c.done[lb] = 1; continue; }
                const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                const double sg = (double)c.sgn[lb];
                const int n = step_grid_steps(-sg * tb[iv], -sg * tb[iv - 1], cfg.step, tf32);
                c.done[lb] = 0;
                c.out_lo[lb] = n; c.out_hi[lb] = 0;
                c.rk_t1[lb] = -sg * tb[iv];
                c.fin[lb] = 0;
                if ((long long)n > cfg.max_steps) { c.st[lb] = PHX_ERR_MAX_STEPS; c.done[lb] = 1; }   // budget per interval
            }
            int active = count_active();
            while (active > 0 && !x.aborted) {
                for (int lb = tid; lb < Bt; lb += blockDim.x) {
                    if (c.done[lb]) continue;
                    const TimeRow tb = trowT(t, T, cfg, shared ? 0 : grp * Bt + lb);
                    const double sg = (double)c.sgn[lb];
                    const int k = c.out_hi[lb], n = c.out_lo[lb];
                    const double g0 = c.rk_t1[lb];
                    const double g1 = step_grid_at(-sg * tb[iv], -sg * tb[iv - 1], cfg.step, tf32, n, k + 1);
                    c.rk_t0[lb] = g0; c.rk_t1[lb] = g1;
                    c.dtf[lb] = tf32 ? ((float)g1 - (float)g0) : (float)(g1 - g0);
                    c.out_hi[lb] = k + 1;
                    c.fin[lb] = (k + 1 >= n) ? 1 : 0;
                }
                __syncthreads();
                for (int st = 0; st < S; ++st) eval_aug(3, st, iv, st, 0);
                __syncthreads();
                for (int lb = tid; lb < Bt; lb += blockDim.x) {
                    const bool act = !c.done[lb];
                    const float dtl = c.dtf[lb];
                    for (int j = 0; j < 8; ++j)
                        wq[lb * 8 + j] = (act && j < S) ? c.sgn[lb] * fixed_weight(cfg.method, j, dtl) : 0.f;
                    if (act) { c.nsteps[lb] += 1; c.nfe[lb] += S; }
                }
                __syncthreads();
                if (want_grads) phaseG(S);
                for (int s = 0; s < d.TPW; ++s) {
                    const int ttl = wv * d.TPW + s;
                    if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                    const int lb = ttl * 16 + li;
                    const int b = grp * Bt + lb;
                    const float dtl = c.dtf[lb];
                    const bool act = !c.done[lb];
                    const int fin = c.fin[lb];
                    if (!__any(act)) continue;
                    for (int bl = 0; bl < nbl; ++bl) {
                        float x0[2][8], k0[2][8], k1[2][8], k2[2][8], k3[2][8], gy8[8], ys8[8];
                        {   // jump data of the trajectories whose grid ends with this step (adjoint.py:152-154)
                            const long long ro = (long long)(iv - 1) * d.BN + (long long)b * N;
                            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                            row_load8(grad_y, ro, g0, N, (b < B) && fin == 1, 0.f, gy8);
                            row_load8(y_saved, ro, g0, N, (b < B) && fin == 1, 0.5f, ys8);
                        }
#pragma unroll
                        for (int h = 0; h < 2; ++h) {   // 0: y, 1: a -- the step's own combination of either half
                            const int K = h ? A_KA : A_KY;
                            load8(tptr(h ? A_A0 : A_Y0, ttl, bl), x0[h]);
                            load8(tptr(K, ttl, bl), k0[h]);
                            if (S >= 2) load8(tptr(K + 1, ttl, bl), k1[h]);
                            if (S >= 4) { load8(tptr(K + 2, ttl, bl), k2[h]); load8(tptr(K + 3, ttl, bl), k3[h]); }
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                float x1;
                                if (cfg.method == PHX_EULER) x1 = x0[h][j] + dtl * k0[h][j];
                                else if (cfg.method == PHX_MIDPOINT) x1 = x0[h][j] + dtl * k1[h][j];
                                else x1 = x0[h][j] + (((k0[h][j] + 3.0f * (k1[h][j] + k2[h][j])) + k3[h][j]) * dtl) * 0.125f;
                                x0[h][j] = x1;
                            }
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (fin == 1) { x0[0][j] = ys8[j]; x0[1][j] += gy8[j]; }
                        if (act) {
                            store8(tptr(A_A0, ttl, bl), x0[1]);
                            store8(tptr(A_Y0, ttl, bl), x0[0]);
                        }
                    }
                }
                __syncthreads();
                if (tid < Bt && !c.done[tid] && c.fin[tid]) {
                    c.done[tid] = 1;
                    for (int j = 0; j < 8; ++j) wq[tid * 8 + j] = 0.f;
                }
                active = count_active();
            }
            continue;
        }
        if (cfg.method != PHX_DOPRI5) {
            // ------------------------------------------------------------ fixed grid: one reversed step
            const int S = fixed_nstages(cfg.method);
            for (int st = 0; st < S; ++st) eval_aug(3, st, iv, st, 0);
            __syncthreads();
            for (int lb = tid; lb < Bt; lb += blockDim.x) {
                const bool act = !c.done[lb];
                const float dtl = dt_rev(lb, iv);
                for (int j = 0; j < 8; ++j)
                    wq[lb * 8 + j] = (act && j < S) ? c.sgn[lb] * fixed_weight(cfg.method, j, dtl) : 0.f;
                if (act) { c.nsteps[lb] += 1; c.nfe[lb] += S; }
            }
            __syncthreads();
            if (want_grads) phaseG(S);
            // jump: aug_state[1] = y[i-1]; aug_state[2] += grad_y[i-1]   (adjoint.py:152-154)
            for (int s = 0; s < d.TPW; ++s) {
                const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                const int lb = ttl * 16 + li;
                const int b = grp * Bt + lb;
                const float dtl = dt_rev(lb, iv);
                for (int bl = 0; bl < nbl; ++bl) {
                    float a0[8], k0[8], k1[8], k2[8], k3[8], yn[8], gy8[8];
                    {
                        const long long ro = (long long)(iv - 1) * d.BN + (long long)b * N;
                        const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                        row_load8(grad_y, ro, g0, N, b < B, 0.f, gy8);
                        row_load8(y_saved, ro, g0, N, b < B, 0.5f, yn);
                    }
                    load8(tptr(A_A0, ttl, bl), a0);
                    load8(tptr(A_KA, ttl, bl), k0);
                    if (S >= 2) load8(tptr(A_KA + 1, ttl, bl), k1);
                    if (S >= 4) { load8(tptr(A_KA + 2, ttl, bl), k2); load8(tptr(A_KA + 3, ttl, bl), k3); }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float a1;
                        if (cfg.method == PHX_EULER) a1 = a0[j] + dtl * k0[j];
                        else if (cfg.method == PHX_MIDPOINT) a1 = a0[j] + dtl * k1[j];
                        else a1 = a0[j] + (((k0[j] + 3.0f * (k1[j] + k2[j])) + k3[j]) * dtl) * 0.125f;
                        a0[j] = a1 + gy8[j];
                    }
                    if (!c.done[lb]) {
                        store8(tptr(A_A0, ttl, bl), a0);
                        store8(tptr(A_Y0, ttl, bl), yn);
                    }
                }
            }
            __syncthreads();
            continue;
        }
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
        eval_aug(0, 0, iv, 0, 1);
        // d0 = norm(y0/scale), d1 = norm(f0/scale): slots (0,1) and (2,3)
        norms(nv);
        tm.mark(8);
        if (tid < Bt && !c.done[tid]) {
            c.h0f[tid] = init_h0(nv[0], nv[1]);
            c.d1[tid] = nv[1];
        }
        __syncthreads();
        eval_aug(1, 0, iv, 1, 2);
        norms(nv);
        tm.mark(8);
        if (tid < Bt && !c.done[tid]) {
            const float h0 = c.h0f[tid];
            const float d2 = nv[0] / h0;
            const double dt = init_dt(h0, c.d1[tid], d2);
            c.dt[tid] = dt; c.dtf[tid] = (float)dt; c.nfe[tid] += 2;
            const double t0 = c.rk_t1[tid];
            if (!(t0 + dt > t0)) { c.st[tid] = PHX_ERR_DT_UNDERFLOW; c.done[tid] = 1; }
        }
        int active = count_active();
        while (active > 0 && !x.aborted) {
            for (int st = 1; st <= 6; ++st) eval_aug(2, st, iv, st, st == 6 ? 3 : 0);
            norms(nv);
            tm.mark(8);
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
                double x = 1.0;
                if (acc && u_end <= t1) { fin = 1; x = (u_end - t0) / (t1 - t0); }
                xfin[lb] = x;
                for (int j = 0; j < 8; ++j) {
                    float wj = 0.f;
                    if (acc && j < 7) {
                        double W;
                        if (!fin) W = DP_CSOL64[j];
                        else {
                            const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
                            const double d1 = (j == 0) ? 1.0 : 0.0, d7 = (j == 6) ? 1.0 : 0.0;
                            const double cj = DP_CSOL64[j], mj = DP_CMID64[j];
                            W = x * d1 + x2 * (d7 - 4.0 * d1 - 5.0 * cj + 16.0 * mj) +
                                x3 * (5.0 * d1 - 3.0 * d7 + 14.0 * cj - 32.0 * mj) +
                                x4 * (2.0 * d7 - 2.0 * d1 - 8.0 * cj + 16.0 * mj);
                        }
                        wj = (float)(sg * (double)dtf * W);
                    }
                    wq[lb * 8 + j] = wj;
                }
                const double dtn = optimal_step_size(dt, ratio);
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
            tm.mark(9);
            if (want_grads) phaseG(7);
            // ---- accept pass
            for (int s = 0; s < d.TPW; ++s) {
                const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                const int lb = ttl * 16 + li;
                const int b = grp * Bt + lb;
                const bool adv = !c.done[lb] && c.accept[lb];
                const int fin = c.fin[lb];
                if (!__any(adv)) continue;
                const float dts = c.dtp[lb];
                const InterpX ix = make_interp_x(xfin[lb]);
                for (int bl = 0; bl < nbl; ++bl) {
                    float a0[8], a1[8], f0[8], f1[8], y1[8], ky6[8], kq[5][8];
                    load8(tptr(A_A0, ttl, bl), a0);
                    load8(tptr(A_AS + 6, ttl, bl), a1);
                    load8(tptr(A_KA, ttl, bl), f0);
                    load8(tptr(A_KA + 6, ttl, bl), f1);
                    load8(tptr(A_YS + 6, ttl, bl), y1);
                    load8(tptr(A_KY + 6, ttl, bl), ky6);
#pragma unroll
                    for (int kk = 0; kk < 5; ++kk) {   // DP_CMID[1] == 0: k2 is not read
                        if (kk == 0) zero8(kq[kk]);
                        else load8(tptr(A_KA + 1 + kk, ttl, bl), kq[kk]);
                    }
                    float am[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) am[j] = f0[j] * (dts * DP_CMID[0]);
#pragma unroll
                    for (int kk = 0; kk < 5; ++kk) {
                        const float cf = dts * DP_CMID[kk + 1];
#pragma unroll
                        for (int j = 0; j < 8; ++j) am[j] += kq[kk][j] * cf;
                    }
                    float anew[8], ynew[8], gy8[8], ys8[8];
                    {   // jump data of the trajectories that reach t_{i-1} in this step (adjoint.py:152-154)
                        const long long ro = (long long)(iv - 1) * d.BN + (long long)b * N;
                        const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                        row_load8(grad_y, ro, g0, N, (b < B) && fin == 1, 0.f, gy8);
                        row_load8(y_saved, ro, g0, N, (b < B) && fin == 1, 0.5f, ys8);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        am[j] += f1[j] * (dts * DP_CMID[6]);
                        if (fin == 1) {
                            const float aout = interp_eval(a0[j], a1[j], a0[j] + am[j], f0[j], f1[j], dts, ix);
                            anew[j] = aout + gy8[j];
                            ynew[j] = ys8[j];
                        } else {
                            anew[j] = a1[j];
                            ynew[j] = y1[j];
                        }
                    }
                    if (adv) {
                        store8(tptr(A_A0, ttl, bl), anew);
                        store8(tptr(A_Y0, ttl, bl), ynew);
                        if (fin != 1) {   // FSAL: stage-7 data is stage-1 data of the next step
                            store8(tptr(A_KA, ttl, bl), f1);
                            store8(tptr(A_KY, ttl, bl), ky6);
                            store8(tptr(A_YS, ttl, bl), y1);
                            store8(tptr(A_AS, ttl, bl), a1);
                            if (want_grads) {
                                float sg6[8];
                                load8(tptr(A_SG + 6, ttl, bl), sg6);
                                store8(tptr(A_SG, ttl, bl), sg6);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            tm.mark(10);
            if (tid < Bt && !c.done[tid] && c.fin[tid]) {
                c.done[tid] = 1;
                for (int j = 0; j < 8; ++j) wq[tid * 8 + j] = 0.f;
            }
            active = count_active();
        }
    }

    // ---- results
    __syncthreads();
    for (int s = 0; s < d.TPW; ++s) {
        const int ttl = wv * d.TPW + s;
        if (ttl >= ntg) continue;
        const int b = grp * Bt + ttl * 16 + li;
        for (int bl = 0; bl < nbl; ++bl) {
            float a0[8];
            load8(tptr(A_A0, ttl, bl), a0);
            row_store8(adj_y0, (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B, a0);
        }
    }
    tm.mark(0);
    if (tm.on)
        for (int i = 0; i < 16; ++i) w.prof[(long long)blockIdx.x * 16 + i] = tm.acc[i];
    if (gt == 0)
        for (int lb = tid; lb < Bt; lb += blockDim.x) {
            const int b = grp * Bt + lb;
            if (b < B) {
                status[b] = x.aborted ? (int)PHX_ERR_SYNC_TIMEOUT : c.st[lb];
                nfe_out[b] = c.nfe[lb];
                nsteps_out[b] = c.nsteps[lb];
            }
        }
}

}  // namespace phxk
using phxk::k1_solve_adj;
