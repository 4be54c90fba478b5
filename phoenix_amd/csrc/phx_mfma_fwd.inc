// phx_mfma_fwd.inc -- v1 forward solve: odeint(ODENet, y0, t) with MFMA contractions, LDS-resident
// weights and group-local hidden-vector exchange (see phx_mfma_common.inc for the decomposition).
// Same algorithm / reference citations as k_solve_fwd in phx_engine.hip.
namespace {

enum { V_Y0 = 0, V_YS = 1, V_K0 = 2, V_J = 9 };  // private state vectors: Y0, stage input, K0..K6 (+ partial j, chunked)
constexpr int NVEC_FWD = 9;
constexpr int NVEC_FWD_CH = 10;

// CH: the hidden layer is processed in d.HC chunks of d.Hc rows (H > 128: one chunk's weights fit in LDS at a
// time).  The RHS is a sum over hidden rows, so chunk c contributes its own hidden rows to the exchange (P1) and
// its own partial j (P2); the chunk left resident by P1 is the first one P2 uses, and vice versa, so every
// evaluation re-stages each chunk but one exactly once (= the 4P weight bytes of the algorithmic count).
}  // namespace
namespace phxk {   // external linkage: instantiated in phx_v1.hip, launched from phx_engine.hip
template <int HT, int MAXT, bool CH>
__global__ __launch_bounds__(MAXT) void k1_solve_fwd(Net net, D1 d, W1 w, SolveCfg cfg, const float *__restrict__ y0,
                                                    const double *__restrict__ t, float *sol, int *status,
                                                    int *nfe_out, int *nsteps_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, H = d.H, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G;
    const int HC = CH ? d.HC : 1, Hc = CH ? d.Hc : H;     // hidden chunks, rows per (full) chunk
    const int BLKF = blk_floats_ch(HT, Hc);   // slots are float4-copyable packed images (k1_pack_images)
    const int RGOFF = BLKF - 32;                           // relu(gene_multipliers) of a block slot
    const bool shared = cfg.control == PHX_CTRL_SHARED;   // host: one batch group per call (TG == 1 unless d.Bcall > 0)
    // row of the caller's arrays behind local trajectory lb of this group (B = none: padding of the last tile)
    auto rowof = [&](int lb) -> int { return d.Bcall > 0 ? (lb < d.Bcall ? grp * d.Bcall + lb : B) : grp * Bt + lb; };
    Ctl c = carve_ctl(lds + (long long)d.NB * BLKF, Bt);
    const int F2 = 2 * HT, F2T = F2 * HC;                  // hidden fragment tiles per chunk / per trajectory tile
    const int RH = ntg * F2T * 4;      // hidden rows of one exchange; norm rows follow
    const int R = RH + ntg;
    Xchg x{w.part + (long long)grp * G * R * 64, w.zbuf + (long long)grp * R * 64, 0, w.abort_flag, 0u, G, gt, R, false};

    SegTimer tm;
    tm.start(w.prof != nullptr, c.tacc);
    stage_images(w.wimg, lds, blk0, nbl, 0, HC, BLKF);
    int resident = 0;                  // hidden chunk whose weights are in LDS (workgroup uniform)
    auto hc_of = [&](int ch) -> int { return min(Hc, H - ch * Hc); };
    auto ensure = [&](int ch, int seg) {
        if (!CH || resident == ch) return;
        tm.mark(seg);
        __syncthreads();               // every wave is done with the previous chunk's weights
        stage_images(w.wimg, lds, blk0, nbl, ch, HC, BLKF);
        __syncthreads();
        resident = ch;
        tm.mark(15);   // weight re-staging of a hidden chunk
    };
    // chunk visited at position ci of a pass that starts with the chunk `r0` left resident by the previous pass
    auto chunk_at = [&](int r0, int ci) -> int { return ci == 0 ? r0 : (ci <= r0 ? ci - 1 : ci); };

    // lane-constant LDS offsets of the two weight-fragment forms
    const int offR = li * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = 4 * lq * LROW + gmapC(li, 0);
    offC[1] = 4 * lq * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * d.nvec * tiles_wg * 512;
    auto tptr = [&](int v, int ttl, int bl) -> float * {
        return wgbase + (((long long)v * tiles_wg + (ttl * d.NB + bl)) * 64 + lane) * 8;
    };

    // ---- controllers (replicated in every workgroup of the group; deterministic => identical)
    for (int lb = tid; lb < Bt; lb += blockDim.x) {
        const int b = rowof(lb);
        const bool vb = b < B;
        const int cbsrc = shared ? grp : (vb ? b : 0);
        const TimeRow tb = trowT(t, T, cfg, cbsrc);
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
        c.accept[lb] = 0; c.fin[lb] = 0;
    }
    // ---- initial state: Y0 tiles <- y0, sol[0] <- y0
    for (int s = 0; s < d.TPW; ++s) {
        const int ttl = wv * d.TPW + s;
        if (ttl >= ntg) continue;
        const int b = rowof(ttl * 16 + li);
        for (int bl = 0; bl < nbl; ++bl) {
            float x[8];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
            row_load8(y0, (long long)b * N, g0, N, b < B, 0.5f, x);
            row_store8(sol, (long long)b * N, g0, N, b < B, x);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g0 + j >= N) x[j] = 0.5f;   // padding genes: a = l = 0
            store8(tptr(V_Y0, ttl, bl), x);
        }
    }
    __syncthreads();
    tm.mark(6);   // init: weight staging + y0 load

    auto count_active = [&]() -> int {   // workgroup-uniform
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int lb = 0; lb < Bt; ++lb) n += c.done[lb] ? 0 : 1;
            c.misc[0] = n;
        }
        __syncthreads();
        return c.misc[0];
    };
    const bool stepped = cfg.method != PHX_DOPRI5 && cfg.step > 0.0;   // options["step_size"]: sub-steps, dt per trajectory
    auto dt_of = [&](int lb, int i) -> float {   // fixed-grid dt of interval i (solvers.py:85-87)
        if (stepped) return c.dtf[lb];           // ... or of the trajectory's running grid step
        const int b = rowof(lb);
        const TimeRow tb = trowT(t, T, cfg, shared ? grp : min(b, B - 1));
        const double sg = (double)c.sgn[lb];
        const double s0 = sg * tb[i], s1 = sg * tb[i + 1];
        return cfg.t_is_f32 ? ((float)s1 - (float)s0) : (float)(s1 - s0);
    };

    // Reduce-scatter of rows [row0, row0+nrows): a workgroup owns whole rows; its waves split the G
    // members (8 rows in flight each), combine through LDS in a fixed order, wave 0 applies `post`
    // and publishes the reduced row with the current tag.
    auto reduce_rows = [&](int row0, int nrows, auto post) {
        if (G <= 16) {
            // few members: a wave reduces a whole row with ONE batch of loads, the workgroup's waves take its rows
            // in turn -- no LDS combine, no barrier per row (small problems are bound by these round trips)
            for (int u = gt + wv * G; u < nrows; u += G * d.NW) {
                const int row = row0 + u;
                const u64 *rows[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) rows[k] = x.part + ((long long)min(k, G - 1) * R + row) * 64;
                float v[16];
                wait_rows<16>(x, rows, G, lane, v);
                float tot = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) tot += (k < G) ? v[k] : 0.f;
                st_gran(x.zbuf + (long long)row * 64, lane, post(u, tot), x.tag);
            }
            return;
        }
        if (G > 128 && d.NW <= 4) {
            // very wide groups (C5: 230 members): two owned rows per pass, 32 member loads in flight per wave
            for (int u = gt; u < nrows; u += 2 * G) {
                const bool hasB = u + G < nrows;
                const int uB = hasB ? u + G : u;
                float sA = 0.f, sB = 0.f;
                for (int g2 = wv; g2 < G; g2 += d.NW * 16) {
                    const u64 *rows[32];
                    int nv = 0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int gg = g2 + k * d.NW;
                        const long long mb = (long long)min(gg, G - 1) * R;
                        rows[k] = x.part + (mb + row0 + u) * 64;
                        rows[16 + k] = x.part + (mb + row0 + uB) * 64;
                        nv += (gg < G) ? 1 : 0;
                    }
                    float v[32];
                    wait_rows<32>(x, rows, 32, lane, v);   // clamped members are real rows: every entry is valid
#pragma unroll
                    for (int k = 0; k < 16; ++k) { sA += (k < nv) ? v[k] : 0.f; sB += (k < nv) ? v[16 + k] : 0.f; }
                }
                c.wred[(0 * 4 + wv) * 64 + lane] = sA;
                c.wred[(1 * 4 + wv) * 64 + lane] = sB;
                __syncthreads();
                if (wv < 2 && (wv == 0 || hasB)) {   // wave 0 publishes row A, wave 1 row B
                    float tot = 0.f;
                    for (int k = 0; k < d.NW; ++k) tot += c.wred[(wv * 4 + k) * 64 + lane];
                    const int uu = wv == 0 ? u : uB;
                    st_gran(x.zbuf + (long long)(row0 + uu) * 64, lane, post(uu, tot), x.tag);
                }
                __syncthreads();   // the combine buffer is reused by the next pair
            }
            return;
        }
        int wbuf = 0;
        for (int u = gt; u < nrows; u += G) {
            const int row = row0 + u;
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
            // combine through LDS, double buffered: one barrier per row, the other waves already fetch the next row
            // while wave 0 publishes this one
            c.wred[(wbuf * 8 + wv) * 64 + lane] = sacc;
            __syncthreads();
            if (wv == 0) {
                float tot = c.wred[wbuf * 8 * 64 + lane];
                for (int k = 1; k < d.NW; ++k) tot += c.wred[(wbuf * 8 + k) * 64 + lane];
                st_gran(x.zbuf + (long long)row * 64, lane, post(u, tot), x.tag);
            }
            wbuf ^= 1;
        }
        __syncthreads();   // the combine buffers are free again for the next call
    };

    // One RHS evaluation of every trajectory tile of this workgroup.
    //   smode 0: input Y0              1: Y0 + h0*K0          2: dopri5 stage st      3: fixed-grid stage st (interval iv)
    //   kslot: K vector that receives sgn*f  (-1: none)
    //   rmode 0: none  1: d0,d1 (misc.py:62-67)  2: d2 (misc.py:74-77)  3: error ratio (misc.py:89-91)
    auto eval = [&](int smode, int st, int iv, int kslot, int rmode) {
        tm.mark(0);   // everything between evaluations (control, accept pass, init)
        x.tag += 1u;  // hidden-vector exchange of this evaluation
        // ---------------- P1: contraction over this workgroup's genes
        const int r0p1 = resident;
        for (int ci = 0; ci < HC; ++ci) {
        const int ch = CH ? chunk_at(r0p1, ci) : 0;
        ensure(ch, 1);
        const int hc = CH ? hc_of(ch) : H;
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const int lb = ttl * 16 + li;
            const int b = rowof(lb);
            f32x4 accu[HT], accv[HT];
#pragma unroll
            for (int f = 0; f < HT; ++f) { accu[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; accv[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
            float dtl = 0.f;
            if (smode == 1) dtl = c.h0f[lb];
            else if (smode == 2) dtl = c.dtf[lb];
            else if (smode == 3) dtl = dt_of(lb, iv);
            for (int bl = 0; bl < nbl; ++bl) {
                float ys[8];
                if (CH && ci > 0) load8(tptr(V_YS, ttl, bl), ys);   // formed by the first chunk's pass
                else load8(tptr(V_Y0, ttl, bl), ys);
                if (CH && ci > 0) {
                } else if (smode == 1) {
                    float k0[8];
                    load8(tptr(V_K0, ttl, bl), k0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) ys[j] = ys[j] + dtl * k0[j];
                } else if (smode == 2) {
                    // all K tiles of the block are requested back to back (one round trip, not `st`)
                    float kq[6][8];
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) {   // k2 has a structurally zero weight in the last row of the tableau
                            if (st == 6 && kk == 1) zero8(kq[kk]);
                            else load8(tptr(V_K0 + kk, ttl, bl), kq[kk]);
                        }
                    float acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
                    for (int kk = 0; kk < 6; ++kk)
                        if (kk < st) {
                            const float cf = DP_BETA[st - 1][kk] * dtl;
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[j] += kq[kk][j] * cf;
                        }
#pragma unroll
                    for (int j = 0; j < 8; ++j) ys[j] = ys[j] + acc[j];
                } else if (smode == 3 && st > 0) {
                    const float third = (float)(1.0 / 3.0);
                    float k0[8], k1[8], k2[8];
                    load8(tptr(V_K0, ttl, bl), k0);
                    if (cfg.method == PHX_MIDPOINT) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) ys[j] = ys[j] + k0[j] * (0.5f * dtl);
                    } else if (st == 1) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) ys[j] = ys[j] + (dtl * k0[j]) * third;
                    } else if (st == 2) {
                        load8(tptr(V_K0 + 1, ttl, bl), k1);
#pragma unroll
                        for (int j = 0; j < 8; ++j) ys[j] = ys[j] + dtl * (k1[j] - k0[j] * third);
                    } else {
                        load8(tptr(V_K0 + 1, ttl, bl), k1);
                        load8(tptr(V_K0 + 2, ttl, bl), k2);
#pragma unroll
                        for (int j = 0; j < 8; ++j) ys[j] = ys[j] + dtl * ((k0[j] - k1[j]) + k2[j]);
                    }
                }
                if (!(CH && ci > 0)) store8(tptr(V_YS, ttl, bl), ys);
                float av[8], lv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                    const bool ok = (b < B) && (gene < N);
                    float a = 0.f, l = 0.f;
                    if (ok) act_pair_fast(ys[j], a, l);
                    av[j] = a; lv[j] = l;
                }
                const float *Wb = lds + (long long)bl * BLKF + offR;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        accu[f] = mfma4(Wb[f * 16 * LROW + j], av[j], accu[f]);
                        accv[f] = mfma4(Wb[(hc + f * 16) * LROW + j], lv[j], accv[f]);
                    }
                }
            }
            u64 *pp = x.part + ((long long)gt * R + ((long long)ttl * F2T + ch * F2) * 4) * 64;
#pragma unroll
            for (int f = 0; f < HT; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    st_gran(pp + ((long long)f * 4 + r) * 64, lane, accu[f][r], x.tag);
                    st_gran(pp + ((long long)(HT + f) * 4 + r) * 64, lane, accv[f][r], x.tag);
                }
        }
        }
        tm.mark(1);   // P1
        reduce_rows(0, RH, [&](int u, float tot) -> float {
            const int r = u & 3, f2t = (u >> 2) % F2T, ch = f2t / F2, f2 = f2t % F2;
            const int rowl = 16 * (f2 % HT) + 4 * lq + r;
            if (rowl >= (CH ? hc_of(ch) : H)) return 0.f;
            const int row = ch * Hc + rowl;
            return (f2 < HT) ? tot + net.bs[row] : expf(tot + net.bp[row]);
        });
        tm.mark(3);   // reduce-scatter (incl. waiting for the members' rows)
        // ---------------- P2: expansion back to genes, RK bookkeeping, norm partial sums
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
            const int b = rowof(lb);
            float zr[2 * HT][4];
            // 16 rows (four fragments) per batch: fewer dependent round trips than fragment pairs
#pragma unroll
            for (int f2 = 0; f2 < 2 * HT; f2 += 4) {
                constexpr int FL = 2 * HT;
                const u64 *rows[16];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    rows[k] = x.zbuf + ((long long)(ttl * F2T + ch * F2 + min(f2 + (k >> 2), FL - 1)) * 4 + (k & 3)) * 64;
                float v[16];
                wait_rows<16>(x, rows, min(16, (FL - f2) * 4), lane, v);
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (f2 + (k >> 2) < FL) zr[f2 + (k >> 2)][k & 3] = v[k];
            }
            if (s == 0 && firstc) tm.mark(4);   // waiting for the reduced hidden vector
            const float sg = c.sgn[lb];
            float dtl = 0.f;
            if (smode == 2) dtl = c.dtf[lb];
            float r0 = 0.f, r1 = 0.f;
            for (int bl = 0; bl < nbl; ++bl) {
                const float *Wb = lds + (long long)bl * BLKF;
                // request every state tile this block needs before the MFMA chain (latency under compute)
                float ys[8], y0v[8], k0[8], kq[6][8], jp[8];
                if (CH && !firstc) load8(tptr(V_J, ttl, bl), jp);
                if (lastc) {
                    load8(tptr(V_YS, ttl, bl), ys);
                    if (rmode >= 2) load8(tptr(V_Y0, ttl, bl), y0v);
                    if (rmode == 2) load8(tptr(V_K0, ttl, bl), k0);
                    if (rmode == 3) {
#pragma unroll
                        for (int kk = 0; kk < 6; ++kk) {   // DP_CERR[1] == 0: k2 is not read
                            if (kk == 1) zero8(kq[kk]);
                            else load8(tptr(V_K0 + kk, ttl, bl), kq[kk]);
                        }
                    }
                }
                float jv[8];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const float *Wc = Wb + offC[s2];
#pragma unroll
                    for (int f2 = 0; f2 < 2 * HT; ++f2) {
                        const int rb = (f2 < HT) ? 2 * hc + 16 * f2 : 3 * hc + 16 * (f2 - HT);
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc = mfma4(Wc[(rb + r) * LROW], zr[f2][r], acc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) jv[4 * s2 + r] = acc[r];
                }
                if (CH) {   // j is a sum over the hidden chunks: carry the partial through the private tile V_J
                    if (!firstc) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) jv[j] += jp[j];
                    }
                    if (!lastc) { store8(tptr(V_J, ttl, bl), jv); continue; }
                }
                float kv[8];
                const float *rg = Wb + RGOFF;
#pragma unroll
                for (int j = 0; j < 8; ++j) kv[j] = sg * (rg[gmap(lq, j)] * (jv[j] - ys[j]));
                if (kslot >= 0) store8(tptr(V_K0 + kslot, ttl, bl), kv);
                if (rmode != 0) {
                    float ksum[8];
                    if (rmode == 3) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) ksum[j] = 0.f;
#pragma unroll
                        for (int kk = 0; kk < 6; ++kk) {
                            const float cf = dtl * DP_CERR[kk];
#pragma unroll
                            for (int j = 0; j < 8; ++j) ksum[j] += kq[kk][j] * cf;
                        }
                        const float cf6 = dtl * DP_CERR[6];
#pragma unroll
                        for (int j = 0; j < 8; ++j) ksum[j] += kv[j] * cf6;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                        if (!((b < B) && (gene < N))) continue;
                        if (rmode == 1) {
                            const float scale = cfg.atol + fabsf(ys[j]) * cfg.rtol;
                            const float q0 = ys[j] / scale, q1 = kv[j] / scale;
                            r0 += q0 * q0; r1 += q1 * q1;
                        } else if (rmode == 2) {
                            const float scale = cfg.atol + fabsf(y0v[j]) * cfg.rtol;
                            const float q0 = (kv[j] - k0[j]) / scale;
                            r0 += q0 * q0;
                        } else {
                            const float tol = cfg.atol + cfg.rtol * fmaxf(fabsf(y0v[j]), fabsf(ys[j]));
                            const float q0 = ksum[j] / tol;
                            r0 += q0 * q0;
                        }
                    }
                }
            }
            if (rmode != 0 && lastc) {
                // norm row of this trajectory tile: lane (slot = lq, trajectory li)
                r0 = sum_over_q(r0);
                r1 = sum_over_q(r1);
                st_gran(x.part + ((long long)gt * R + RH + ttl) * 64, lane, lq == 0 ? r0 : (lq == 1 ? r1 : 0.f), x.tag + 1u);
            }
        }
        }
        if (rmode != 0) x.tag += 1u;   // the norm rows form their own exchange
        tm.mark(5);   // P2
    };

    // norms of every controller: reduce the norm rows across the group, fan them back out through LDS
    auto norms = [&](int nslots, float *out /* per-thread result [nslots] */) {
        reduce_rows(RH, ntg, [&](int, float tot) -> float { return tot; });
        for (int s = 0; s < d.TPW; ++s) {
            const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
            const u64 *rows[1] = {x.zbuf + (long long)(RH + ttl) * 64};
            float v[1];
            wait_rows<1>(x, rows, 1, lane, v);
            c.nrm[ttl * 64 + lane] = v[0];
        }
        __syncthreads();
        double v2[2] = {0.0, 0.0};
        if (tid < Bt && (rowof(tid)) < B)
            for (int k = 0; k < nslots; ++k) v2[k] = (double)c.nrm[(tid >> 4) * 64 + k * 16 + (tid & 15)];
        if (!shared) {
            for (int k = 0; k < nslots; ++k) out[k] = sqrtf((float)(v2[k] / (double)N));
            __syncthreads();
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
    };

    if (stepped) {
        // ------------------------------------------------------------------ fixed grid with a step size (solvers.py:59-103)
        // One grid per trajectory, anchored at its t[0]; a step writes the outputs it reaches or passes (the state at a
        // grid point, else the linear interpolant); a trajectory whose grid has ended is masked like `done` in the dopri5
        // arm.  Intermediate states never leave the private tiles.
        const int S = fixed_nstages(cfg.method);
        const bool tf32 = cfg.t_is_f32 != 0;
        for (int lb = tid; lb < Bt; lb += blockDim.x) {
            c.dtf[lb] = 0.f;
            if (c.done[lb]) continue;
            const TimeRow tb = trowT(t, T, cfg, shared ? grp : rowof(lb));
            const double sg = (double)c.sgn[lb];
            c.nsiv[lb] = step_grid_steps(sg * tb[0], sg * tb[T - 1], cfg.step, tf32);
            // max_num_steps: a budget of grid steps per call (a tiny step would hold the device for hours otherwise)
            if ((long long)c.nsiv[lb] > cfg.max_steps) { c.st[lb] = PHX_ERR_MAX_STEPS; c.done[lb] = 1; }
        }
        int active = count_active();
        while (active > 0 && !x.aborted) {
            for (int lb = tid; lb < Bt; lb += blockDim.x) {
                if (c.done[lb]) continue;
                const TimeRow tb = trowT(t, T, cfg, shared ? grp : rowof(lb));
                const double sg = (double)c.sgn[lb];
                const int k = c.nsteps[lb], n = c.nsiv[lb];
                const double g0 = c.rk_t1[lb];
                const double g1 = step_grid_at(sg * tb[0], sg * tb[T - 1], cfg.step, tf32, n, k + 1);
                c.rk_t0[lb] = g0; c.rk_t1[lb] = g1;
                c.dtf[lb] = tf32 ? ((float)g1 - (float)g0) : (float)(g1 - g0);
                int oi = c.out_idx[lb];
                c.out_lo[lb] = oi;
                while (oi < T && sg * tb[oi] <= g1) ++oi;
                c.out_hi[lb] = oi; c.out_idx[lb] = oi;
                c.nsteps[lb] = k + 1; c.nfe[lb] += S;
                c.fin[lb] = (k + 1 >= n) ? 1 : 0;
            }
            __syncthreads();
            for (int st = 0; st < S; ++st) eval(3, st, 0, st, 0);
            for (int s = 0; s < d.TPW; ++s) {
                const int ttl = wv * d.TPW + s;
                if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                const int lb = ttl * 16 + li;
                const int b = rowof(lb);
                const float dtl = c.dtf[lb];
                const bool active1 = !c.done[lb];
                if (!__any(active1)) continue;
                const int lo = c.out_lo[lb], hi = c.out_hi[lb];
                const double g0 = c.rk_t0[lb], g1 = c.rk_t1[lb];
                const double sg = (double)c.sgn[lb];
                const TimeRow tb = trowT(t, T, cfg, shared ? grp : min(b, B - 1));
                for (int bl = 0; bl < nbl; ++bl) {
                    float yv[8], y1[8], k0[8], k1[8], k2[8], k3[8];
                    load8(tptr(V_Y0, ttl, bl), yv);
                    load8(tptr(V_K0, ttl, bl), k0);
                    if (S >= 2) load8(tptr(V_K0 + 1, ttl, bl), k1);
                    if (S >= 4) { load8(tptr(V_K0 + 2, ttl, bl), k2); load8(tptr(V_K0 + 3, ttl, bl), k3); }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (cfg.method == PHX_EULER) y1[j] = yv[j] + dtl * k0[j];
                        else if (cfg.method == PHX_MIDPOINT) y1[j] = yv[j] + dtl * k1[j];
                        else y1[j] = yv[j] + (((k0[j] + 3.0f * (k1[j] + k2[j])) + k3[j]) * dtl) * 0.125f;
                    }
                    if (active1) {
                        for (int jo = lo; jo < hi; ++jo) {   // _linear_interp (solvers.py:97-103)
                            const double tj = sg * tb[jo];
                            float ov[8];
                            if (tj == g0) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) ov[j] = yv[j];
                            } else if (tj == g1) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) ov[j] = y1[j];
                            } else {
                                const float slope = tf32 ? ((float)tj - (float)g0) / ((float)g1 - (float)g0)
                                                         : (float)((tj - g0) / (g1 - g0));
#pragma unroll
                                for (int j = 0; j < 8; ++j) ov[j] = yv[j] + slope * (y1[j] - yv[j]);
                            }
                            row_store8(sol, (long long)jo * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B,
                                       ov);
                        }
                        store8(tptr(V_Y0, ttl, bl), y1);   // per-lane select: a finished trajectory keeps its state
                    }
                }
            }
            __syncthreads();
            if (tid < Bt && !c.done[tid] && c.fin[tid]) c.done[tid] = 1;
            active = count_active();
        }
    } else if (cfg.method != PHX_DOPRI5) {
        // ------------------------------------------------------------------ fixed grid (solvers.py:77-95)
        const int S = fixed_nstages(cfg.method);
        for (int i = 0; i + 1 < T; ++i) {
            for (int st = 0; st < S; ++st) eval(3, st, i, st, 0);
            for (int s = 0; s < d.TPW; ++s) {
                const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                const int lb = ttl * 16 + li;
                const int b = rowof(lb);
                const float dtl = dt_of(lb, i);
                const bool active = !c.done[lb];
                for (int bl = 0; bl < nbl; ++bl) {
                    float yv[8], k0[8], k1[8], k2[8], k3[8];
                    load8(tptr(V_Y0, ttl, bl), yv);
                    load8(tptr(V_K0, ttl, bl), k0);
                    if (S >= 2) load8(tptr(V_K0 + 1, ttl, bl), k1);
                    if (S >= 4) { load8(tptr(V_K0 + 2, ttl, bl), k2); load8(tptr(V_K0 + 3, ttl, bl), k3); }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float y1;
                        if (cfg.method == PHX_EULER) y1 = yv[j] + dtl * k0[j];
                        else if (cfg.method == PHX_MIDPOINT) y1 = yv[j] + dtl * k1[j];
                        else y1 = yv[j] + (((k0[j] + 3.0f * (k1[j] + k2[j])) + k3[j]) * dtl) * 0.125f;
                        yv[j] = y1;
                    }
                    row_store8(sol, (long long)(i + 1) * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N,
                               active && b < B, yv);
                    store8(tptr(V_Y0, ttl, bl), yv);
                }
            }
        }
        __syncthreads();
        for (int lb = tid; lb < Bt; lb += blockDim.x)
            if (!c.done[lb]) { c.nsteps[lb] = T - 1; c.nfe[lb] = S * (T - 1); }
    } else {
        // ------------------------------------------------------------------ dopri5
        float nv[2];
        eval(0, 0, 0, 0, 1);
        norms(2, nv);
        tm.mark(8);   // norm exchange
        if (tid < Bt && !c.done[tid]) {
            c.h0f[tid] = init_h0(nv[0], nv[1]);
            c.d1[tid] = nv[1];
        }
        __syncthreads();
        eval(1, 0, 0, -1, 2);
        norms(1, nv);
        tm.mark(8);
        if (tid < Bt && !c.done[tid]) {
            const float h0 = c.h0f[tid];
            const float d2 = nv[0] / h0;
            const double dt = init_dt(h0, c.d1[tid], d2);
            c.dt[tid] = dt; c.dtf[tid] = (float)dt; c.nfe[tid] = 2;
            const double t0 = c.rk_t1[tid];
            if (!(t0 + dt > t0)) { c.st[tid] = PHX_ERR_DT_UNDERFLOW; c.done[tid] = 1; }
        }
        int active = count_active();
        while (active > 0 && !x.aborted) {
            for (int st = 1; st <= 6; ++st) eval(2, st, 0, st, st == 6 ? 3 : 0);
            norms(1, nv);
            tm.mark(8);
            // ---- controller (rk_common.py:150-220)
            if (tid < Bt && !c.done[tid]) {
                const int lb = tid;
                const int b = rowof(lb);
                const TimeRow tb = trowT(t, T, cfg, shared ? grp : b);
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
                const double dtn = optimal_step_size(dt, ratio);
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
            tm.mark(9);   // controller
            // ---- accept pass: dense output (interp.py) + FSAL advance
            for (int s = 0; s < d.TPW; ++s) {
                const int ttl = wv * d.TPW + s;
            if (ttl >= ntg) continue;   // helper wave: no trajectory tile of its own, it only serves the exchange
                const int lb = ttl * 16 + li;
                const int b = rowof(lb);
                const bool adv = !c.done[lb] && c.accept[lb];
                const int lo = c.out_lo[lb], hi = c.out_hi[lb];
                const double t0 = c.rk_t0[lb], t1 = c.rk_t1[lb];
                const float dts = c.dtp[lb];
                const double sg = (double)c.sgn[lb];
                const TimeRow tb = trowT(t, T, cfg, shared ? grp : min(b, B - 1));
                for (int bl = 0; bl < nbl; ++bl) {
                    if (!__any(adv)) continue;
                    float y0v[8], y1v[8], f0[8], f1[8];
                    load8(tptr(V_Y0, ttl, bl), y0v);
                    load8(tptr(V_YS, ttl, bl), y1v);
                    load8(tptr(V_K0, ttl, bl), f0);
                    load8(tptr(V_K0 + 6, ttl, bl), f1);
                    if (__any(adv && hi > lo)) {
                        float ym[8], kq[5][8];
#pragma unroll
                        for (int kk = 0; kk < 5; ++kk) {   // DP_CMID[1] == 0: k2 is not read
                            if (kk == 0) zero8(kq[kk]);
                            else load8(tptr(V_K0 + 1 + kk, ttl, bl), kq[kk]);
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) ym[j] = f0[j] * (dts * DP_CMID[0]);
#pragma unroll
                        for (int kk = 0; kk < 5; ++kk) {
                            const float cf = dts * DP_CMID[kk + 1];
#pragma unroll
                            for (int j = 0; j < 8; ++j) ym[j] += kq[kk][j] * cf;
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) ym[j] += f1[j] * (dts * DP_CMID[6]);
                        if (adv) {
                            for (int jo = lo; jo < hi; ++jo) {
                                const double x = (sg * tb[jo] - t0) / (t1 - t0);
                                const InterpX ix = make_interp_x(x);
                                float ov[8];
#pragma unroll
                                for (int j = 0; j < 8; ++j)
                                    ov[j] = interp_eval(y0v[j], y1v[j], y0v[j] + ym[j], f0[j], f1[j], dts, ix);
                                row_store8(sol, (long long)jo * d.BN + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N,
                                           b < B, ov);
                            }
                        }
                    }
                    if (adv) {   // per-lane select: rejected / finished trajectories keep their state
                        store8(tptr(V_Y0, ttl, bl), y1v);
                        store8(tptr(V_K0, ttl, bl), f1);
                    }
                }
            }
            __syncthreads();
            tm.mark(10);  // accept pass
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
}

}  // namespace phxk
using phxk::k1_solve_fwd;
