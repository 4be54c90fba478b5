// phx_mfma_bp.inc -- backward pass of `odeint` with a fixed-grid method (euler / midpoint / rk4): backpropagation through
// the solver's own steps (the DISCRETE adjoint), one persistent launch.  Not the continuous adjoint of phx_mfma_adj2.inc:
// this kernel differentiates the numbers the forward pass produced, whatever the step (torchdiffeq/_impl/odeint.py:30-74
// returns an autograd-tracked solution; fixed_grid.py:6-38, rk_common.py:96-103 are the steps differentiated here).
//
// One grid step y -> y' of length dt with stage inputs Y_1..Y_s (Y_i = y + dt sum_{j<i} a_ij k_j, k_j = f(Y_j),
// y' = y + dt sum b_i k_i), cotangent c of y':
//     for i = s .. 1:   w_i = dt (b_i c + sum_{j>i} a_ji z_j),   z_i = J(Y_i)^T w_i,   dtheta += P(Y_i)^T w_i
//     cotangent of y = c + sum_i z_i
// so a step costs s - 1 plain evaluations (Y_2..Y_s from the step's start state) and s adjoint-type evaluations (hidden
// layer at Y_i, product against w_i, parameter-gradient contraction), every stage with weight 1 in the parameter sum.
//
// Decomposition: the gene-tile x batch-group launch of phx_mfma_common.inc.  A workgroup keeps the weight images of its NB
// gene blocks in LDS; each of its four waves owns ONE 16-trajectory tile and does both halves of an evaluation (expression
// side: a(Y), l(Y) -> u, v -> j = Wa z; cotangent side: q = w relu(g) -> dz = WaT q -> Ws^T du, Wp^T dv).  After staging
// there is no workgroup barrier: a wave meets the G - 1 workgroups that hold the other gene tiles of ITS trajectory tile
// through tagged granule rows only (one exchange per evaluation, bounded polls with the abort flag: wait_members).
//
// The grid.  Without a step size the grid is t itself and the start state of step k is y_saved[k].  With
// options["step_size"] the grid is phx_odeint_stepped's (one grid per trajectory anchored at t[0], last step clipped,
// outputs between grid points linearly interpolated): the kernel first re-runs the forward grid from y_saved[0] and writes
// the start state of every step into the checkpoint region of the workspace ([K][B][N] floats), then sweeps back over
// them.  An output at fraction th of step k sends (1 - th) grad to grid state k and th grad to grid state k + 1; an output
// on a grid point sends its whole cotangent there (_linear_interp returns that state itself, solvers.py:97-103).
// Time is solver time s = sgn t as in k1_solve_fwd: k = sgn f, dt > 0, formed in the same rounding.
namespace {

constexpr int BP_NW = 4;      // waves per workgroup: one per SIMD, up to 512 registers each (HT = 8 keeps 32 accumulators)
constexpr int NVEC_BP = 18;   // private state vectors (tile-native scratch)
__device__ __forceinline__ int bpC() { return 0; }           // running cotangent
__device__ __forceinline__ int bpY(int s) { return 1 + s; }  // stage inputs (bpY(0): start state of the step)
__device__ __forceinline__ int bpW(int s) { return 5 + s; }  // stage cotangents w_i
__device__ __forceinline__ int bpK(int s) { return 9 + s; }  // k_i = sgn f(Y_i)
__device__ __forceinline__ int bpZ(int s) { return 13 + s; } // z_i
__device__ __forceinline__ int bpP() { return 17; }          // output cotangents owed to the step's start state

template <int HT>
__global__ __launch_bounds__(64 * BP_NW) void k1_solve_bp(Net net, D1 d, W1 w, SolveCfg cfg, const double *__restrict__ t,
                                                           const float *__restrict__ y_saved,
                                                           const float *__restrict__ grad_y, float *adj_y0, int *status,
                                                           int *nfe_out, int *nsteps_out, int want_grads, long long PP,
                                                           float *ckpt)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, H = d.H, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G;
    const int BLKF = blk_floats_ch(HT, H);
    const int RGOFF = BLKF - 32;
    constexpr int F4 = 4 * HT, F2 = 2 * HT;
    const int R = ntg * F4 * 4;             // exchange rows of a workgroup: per tile [u | v | dz_u | dz_p] x HT x 4
    u64 *part = w.part + (long long)grp * G * R * 64;
    u64 *zb = w.zbuf + (long long)grp * R * 64;
    Xg2 x{w.abort_flag, false};
    unsigned int tag = 0u;

    stage_images(w.wimg, lds, blk0, nbl, 0, 1, BLKF);
    __syncthreads();                        // the ONLY workgroup barrier: from here on every wave runs on its own
    if (wv >= ntg) return;                  // wave without a tile (last group of a small batch)
    const int ttl = wv;

    const int offR = li * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = 4 * lq * LROW + gmapC(li, 0);
    offC[1] = 4 * lq * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * NVEC_BP * tiles_wg * 512;
    const unsigned lane8 = lane * 8;
    auto tptr = [&](int v, int bl) -> float * {
        return wgbase + (unsigned)((v * tiles_wg + ttl * d.NB + bl) * 512) + lane8;
    };
    // wave-private transposed hidden rows of the four stage slots: [workgroup][wave][slot][F4][64] float4
    float *hqbase = w.hq + ((long long)blockIdx.x * BP_NW + wv) * 4 * F4 * 256;
    auto hqp = [&](int slot, int f) -> float4 * {
        return reinterpret_cast<float4 *>(hqbase + ((unsigned)((slot * F4 + f) * 256) + (unsigned)lane * 4));
    };
    float *dth = w.dtheta + (long long)(grp * BP_NW + wv) * PP;   // this trajectory tile's parameter-gradient partial
    const long long oWs = 0, oWp = (long long)H * N, oWa = 2LL * H * N, og = 4LL * H * N, obs = og + N, obp = obs + H;

    // ---- this lane's trajectory (lane li <-> trajectory li of the tile; the four lq copies agree) and its grid
    const int b = grp * Bt + ttl * 16 + li;
    const bool vb = b < B;
    const TimeRow tb = trowT(t, T, cfg, vb ? b : 0);
    const bool stepped = cfg.step > 0.0, tf32 = cfg.t_is_f32 != 0;
    const int S = fixed_nstages(cfg.method);
    float sgf = 1.0f;
    int st = PHX_OK;
    if (T >= 2) {
        sgf = (tb[1] < tb[0]) ? -1.0f : 1.0f;
        for (int k = 0; k + 1 < T; ++k)
            if (!((double)sgf * tb[k + 1] > (double)sgf * tb[k])) st = PHX_ERR_BAD_ARG;
    }
    const double sg = (double)sgf;
    const double S0 = sg * tb[0], S1 = sg * tb[T - 1];
    int n = T - 1;                          // grid steps of this trajectory
    if (stepped && T >= 2 && st == PHX_OK) {
        n = step_grid_steps(S0, S1, cfg.step, tf32);
        if ((long long)n > cfg.max_steps) st = PHX_ERR_MAX_STEPS;        // the forward call's budget, same meaning
        else if (n > d.K) st = PHX_ERR_WORKSPACE;                        // more steps than the checkpoint region holds
    }
    const bool ok = vb && st == PHX_OK;     // everything else is carried as a padding trajectory (y = 0.5, cotangent 0)
    if (!ok || T < 2) n = 0;
    int nmax = n;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) nmax = max(nmax, __shfl_xor(nmax, m, 64));
    auto gat = [&](int k) -> double {       // grid point k in solver time
        if (stepped) return step_grid_at(S0, S1, cfg.step, tf32, n, k);
        return sg * tb[min(k, T - 1)];
    };
    auto dt_at = [&](int k) -> float {      // the forward kernel's dt of step k, in its rounding; 0 past the grid's end
        if (k >= n) return 0.f;
        const double g0 = gat(k), g1 = gat(k + 1);
        return tf32 ? ((float)g1 - (float)g0) : (float)(g1 - g0);
    };

    // Reduction of the exchange rows [u0, u1) of this tile that THIS workgroup owns (row u belongs to workgroup u % G):
    // the members' partial rows are summed in member order (deterministic), the reduced row published with the tag.
    auto reduce_owned = [&](int u0, int u1) {
        const int first = u0 + ((gt - u0 % G) + G) % G;
        for (int u = first; u < u1; u += G) {
            float tot = 0.f;
            const u64 *row0 = part + (size_t)u * 64;
            for (int m0 = 0; m0 < G; m0 += 16) {
                const int nv = min(16, G - m0);
                float v[16];
                wait_members<16>(x, row0 + (size_t)m0 * ((size_t)R * 64), (unsigned)(R * 64), nv, tag, lane, v);
#pragma unroll
                for (int m = 0; m < 16; ++m) tot += (m < nv) ? v[m] : 0.f;
            }
            const int r = u & 3, f4 = (u >> 2) % F4, sec = f4 / HT;
            const int row = 16 * (f4 % HT) + 4 * lq + r;
            float val = tot;                                   // du, dz_p (consumer: dv = dz_p * z_p)
            if (row >= H) val = 0.f;
            else if (sec == 0) val = tot + net.bs[row];        // z_u
            else if (sec == 1) val = expf(tot + net.bp[row]);  // z_p
            st_gran(zb + (size_t)u * 64, lane, val, tag);
        }
    };

    // -----------------------------------------------------------------------------------------------------------
    // One evaluation of this wave's tile.  ADJ = 0: plain, k = sgn f(Y) -> vk.  ADJ = 1: adjoint-type, also
    // z = sgn J(Y)^T w -> vz and the transposed hidden rows of stage slot `slot` for the gradient contraction.
    // form(bl, ys, ws): fills the stage input (and cotangent) tile of gene block bl; eval stores them to vy / vw.
    // -----------------------------------------------------------------------------------------------------------
    auto eval = [&](auto ADJC, int vy, int vw, int vk, int vz, int slot, auto form) {
        constexpr int ADJ = decltype(ADJC)::value;
        constexpr int NF = ADJ ? F4 : F2;   // hidden tiles exchanged
        tag += 1u;
        {   // ---- P1: contraction over this workgroup's genes
            f32x4 acc[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int bl = 0; bl < nbl; ++bl) {
                const float *Wb = lds + (long long)bl * BLKF;
                const float *rg = Wb + RGOFF;
                float ys[8], ws[8], bop[8], bop2[8], bq[8];
                form(bl, ys, ws);
                store8(tptr(vy, bl), ys);
                if (ADJ) store8(tptr(vw, bl), ws);
                // no masks: a padded gene keeps (Y, w) = (0.5, 0) for the whole solve (its weight columns and relu(g) are
                // zero in the LDS image), where a(Y) = l(Y) = q = 0; a padding trajectory only feeds its own MFMA column
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    act_pair_fast(ys[j], bop[j], bop2[j]);
                    if (ADJ) bq[j] = ws[j] * rg[gmap(lq, j)];
                }
                const float *Wr = Wb + offR;
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        acc[f] = mfma4(Wr[f * 16 * LROW + j], bop[j], acc[f]);
                        acc[HT + f] = mfma4(Wr[(H + f * 16) * LROW + j], bop2[j], acc[HT + f]);
                        if (ADJ) {
                            acc[F2 + f] = mfma4(Wr[(2 * H + 16 * f) * LROW + j], bq[j], acc[F2 + f]);
                            acc[F2 + HT + f] = mfma4(Wr[(3 * H + 16 * f) * LROW + j], bq[j], acc[F2 + HT + f]);
                        }
                    }
            }
            u64 *pp = part + ((size_t)gt * R + (size_t)ttl * F4 * 4) * 64;
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) st_gran(pp + (unsigned)((f * 4 + r) * 64), lane, acc[f][r], tag);
        }
        reduce_owned(ttl * F4 * 4, ttl * F4 * 4 + NF * 4);
        // ---- the tile's reduced hidden rows: z_u | z_p (| du | dz_p), eight rows per batch of loads
        float hr[NF][4];
#pragma unroll
        for (int f0 = 0; f0 < NF; f0 += 2) {
            float v[8];
            wait_members<8>(x, zb + (size_t)((ttl * F4 + f0) * 4) * 64, 64u, 8, tag, lane, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) hr[f0 + (k >> 2)][k & 3] = v[k];
        }
        if (ADJ) {
#pragma unroll
            for (int f = 0; f < HT; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) hr[F2 + HT + f][r] *= hr[HT + f][r];   // dv = dz_p * z_p
            if (want_grads) {   // transposed copies: operands of the products over trajectories
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    float o[4];
                    xpose4(hr[f], o, lane);
                    *hqp(slot, f) = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
        // ---- P2: expansion back to genes
        for (int bl = 0; bl < nbl; ++bl) {
            const float *Wb = lds + (long long)bl * BLKF;
            const float *rg = Wb + RGOFF;
            float ys[8], ws[8], jv[8], p0[8], p1[8];
            load8(tptr(vy, bl), ys);
            if (ADJ) load8(tptr(vw, bl), ws);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float *Wc = Wb + offC[s2];
                f32x4 aj = (f32x4){0.f, 0.f, 0.f, 0.f}, a0 = aj, a1 = aj;
#pragma unroll
                for (int f2 = 0; f2 < F2; ++f2) {   // j = Wa z  (z_u rows then z_p rows)
                    const int rb = (f2 < HT) ? 2 * H + 16 * f2 : 3 * H + 16 * (f2 - HT);
#pragma unroll
                    for (int r = 0; r < 4; ++r) aj = mfma4(Wc[(rb + r) * LROW], hr[f2][r], aj);
                }
                if (ADJ) {                          // Ws^T du, Wp^T dv
#pragma unroll
                    for (int f = 0; f < HT; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            a0 = mfma4(Wc[(16 * f + r) * LROW], hr[ADJ ? F2 + f : 0][r], a0);
                            a1 = mfma4(Wc[(H + 16 * f + r) * LROW], hr[ADJ ? F2 + HT + f : 0][r], a1);
                        }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { jv[4 * s2 + r] = aj[r]; p0[4 * s2 + r] = a0[r]; p1[4 * s2 + r] = a1[r]; }
            }
            float kv[8], zv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float rr = rg[gmap(lq, j)];
                kv[j] = sgf * (rr * (jv[j] - ys[j]));
                if (ADJ) {
                    float da, dl;
                    act_grad_fast2(ys[j], da, dl);
                    zv[j] = sgf * ((p0[j] * da + p1[j] * dl) - ws[j] * rr);
                }
            }
            store8(tptr(vk, bl), kv);
            if (ADJ) store8(tptr(vz, bl), zv);
        }
    };

    // stage input Y_st of the running step (fixed_grid.py:6-38, rk_common.py:96-103), in the forward kernel's rounding
    auto form_y = [&](int st, float dtl, int bl, float *ys) {
        load8(tptr(bpY(0), bl), ys);
        if (st == 0) return;
        float k0[8], k1[8], k2[8];
        load8(tptr(bpK(0), bl), k0);
        const float third = (float)(1.0 / 3.0);
        if (cfg.method == PHX_MIDPOINT) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ys[j] = ys[j] + k0[j] * (0.5f * dtl);
        } else if (st == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ys[j] = ys[j] + (dtl * k0[j]) * third;
        } else if (st == 2) {
            load8(tptr(bpK(1), bl), k1);
#pragma unroll
            for (int j = 0; j < 8; ++j) ys[j] = ys[j] + dtl * (k1[j] - k0[j] * third);
        } else {
            load8(tptr(bpK(1), bl), k1);
            load8(tptr(bpK(2), bl), k2);
#pragma unroll
            for (int j = 0; j < 8; ++j) ys[j] = ys[j] + dtl * ((k0[j] - k1[j]) + k2[j]);
        }
    };
    // the step's result from its start state and its k (the forward kernel's combination)
    auto advance = [&](float dtl, int bl, float *y1) {
        float yv[8], k0[8], k1[8], k2[8], k3[8];
        load8(tptr(bpY(0), bl), yv);
        load8(tptr(bpK(0), bl), k0);
        if (S >= 2) load8(tptr(bpK(1), bl), k1);
        if (S >= 4) { load8(tptr(bpK(2), bl), k2); load8(tptr(bpK(3), bl), k3); }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (cfg.method == PHX_EULER) y1[j] = yv[j] + dtl * k0[j];
            else if (cfg.method == PHX_MIDPOINT) y1[j] = yv[j] + dtl * k1[j];
            else y1[j] = yv[j] + (((k0[j] + 3.0f * (k1[j] + k2[j])) + k3[j]) * dtl) * 0.125f;
        }
    };
    // cotangent w_st of k_st: the transposed tableau applied to the step's cotangent c and the z of the later stages
    auto form_w = [&](int st, float dtl, int bl, float *ws) {
        float c8[8], za[8], zb8[8], zc[8];
        load8(tptr(bpC(), bl), c8);
        if (cfg.method == PHX_EULER) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ws[j] = dtl * c8[j];
        } else if (cfg.method == PHX_MIDPOINT) {
            if (st == 1) {
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = dtl * c8[j];
            } else {
                load8(tptr(bpZ(1), bl), za);
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = (0.5f * dtl) * za[j];
            }
        } else {
            const float third = (float)(1.0 / 3.0), e8 = dtl * 0.125f;
            if (st == 3) {
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = e8 * c8[j];
            } else if (st == 2) {
                load8(tptr(bpZ(3), bl), za);
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = (3.0f * e8) * c8[j] + dtl * za[j];
            } else if (st == 1) {
                load8(tptr(bpZ(3), bl), za);
                load8(tptr(bpZ(2), bl), zb8);
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = (3.0f * e8) * c8[j] + dtl * (zb8[j] - za[j]);
            } else {
                load8(tptr(bpZ(3), bl), za);
                load8(tptr(bpZ(2), bl), zb8);
                load8(tptr(bpZ(1), bl), zc);
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] = e8 * c8[j] + dtl * (za[j] + (zc[j] - zb8[j]) * third);
            }
        }
    };

    // -----------------------------------------------------------------------------------------------------------
    // Parameter gradients of one step: sum over its stage slots of P(Y_i)^T (sgn w_i), added to this tile's partial
    //   cotangent side:  dWs += (sgn du)^T a(Y_i), dWp += (sgn dv)^T l(Y_i), bias gradients
    //   expression side: dWaT += (sgn z)^T (w_i relu(g)), dg += sgn w_i (j - Y_i) with j - Y_i = sgn k_i / relu(g)
    // Per gene block four passes (side x row section) of HT accumulator tiles over the stages.
    // -----------------------------------------------------------------------------------------------------------
    auto quadrature = [&]() {
        float w4[4];   // weight sgn of the four trajectories of this lane's MFMA k-steps
#pragma unroll
        for (int r = 0; r < 4; ++r) w4[r] = __shfl(sgf, 4 * lq + r, 64);
        for (int bl = 0; bl < nbl; ++bl) {
            const float *rg = lds + (long long)bl * BLKF + RGOFF;
            const int gene0 = (blk0 + bl) * 32;
            const float rrc[2] = {rg[gmapC(li, 0)], rg[gmapC(li, 1)]};
            for (int pass = 0; pass < 4; ++pass) {
                const int side = pass >> 1, half = pass & 1;
                f32x4 ga[HT][2];
                float dgn[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) dgn[j] = 0.f;
#pragma unroll
                for (int f = 0; f < HT; ++f) { ga[f][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; ga[f][1] = ga[f][0]; }
                for (int sidx = 0; sidx < S; ++sidx) {
                    float xnat[8], bb[2][4];
                    load8(tptr(side ? bpY(sidx) : bpW(sidx), bl), xnat);
                    if (pass == 0) {
                        float knat[8];
                        load8(tptr(bpK(sidx), bl), knat);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float rr = rg[gmap(lq, j)];
                            dgn[j] += rr > 0.f ? xnat[j] * knat[j] * fast_rcp(rr) : 0.f;
                        }
                    }
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        float xr[4];
                        xpose4(&xnat[4 * s2], xr, lane);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (side == 0) bb[s2][r] = xr[r] * rrc[s2];
                            else {
                                float a, l;
                                act_pair_fast(xr[r], a, l);
                                bb[s2][r] = half ? l : a;
                            }
                        }
                    }
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        const float4 h4 = *hqp(sidx, side * F2 + half * HT + f);
                        const float hd[4] = {w4[0] * h4.x, w4[1] * h4.y, w4[2] * h4.z, w4[3] * h4.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) ga[f][s2] = mfma4(hd[r], bb[s2][r], ga[f][s2]);
                    }
                }
                // accumulators are quad-transposed so that a lane owns four consecutive genes of ONE row
                const long long base = side == 0 ? oWa + (long long)(half ? H : 0) * N : (half ? oWp : oWs);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int gene4 = gene0 + gmapC(li & ~3, s2), rowq = 4 * lq + (li & 3);
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        float a4[4], t0[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) a4[r] = ga[f][s2][r];
                        quad_transpose(a4, t0, lane);
                        const int hrow = 16 * f + rowq;
                        if (hrow < H && gene4 < N) add_store4(dth + base + (long long)hrow * N + gene4, t0, gene4, N, false);
                    }
                }
                if (pass == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float dg = dgn[j];
                        dg += __shfl_xor(dg, 1, 64); dg += __shfl_xor(dg, 2, 64);
                        dg += __shfl_xor(dg, 4, 64); dg += __shfl_xor(dg, 8, 64);
                        const int gene = gene0 + gmap(lq, j);
                        if (li == 0 && gene < N) dth[og + gene] += dg;
                    }
                }
            }
        }
        if (gt == 0) {   // bias gradients: gene independent => only the first gene tile of the group accumulates them
#pragma unroll
            for (int f = 0; f < F2; ++f) {
                float sb = 0.f;
                for (int sidx = 0; sidx < S; ++sidx) {
                    const float4 h4 = *hqp(sidx, F2 + f);
                    sb += w4[0] * h4.x + w4[1] * h4.y + w4[2] * h4.z + w4[3] * h4.w;
                }
                sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
                const int hid = 16 * (f % HT) + li;
                const long long o = (f < HT ? obs : obp) + hid;
                if (lq == 0 && hid < H) dth[o] += sb;
            }
        }
    };

    const long long ckrow = (long long)B * N;   // floats per checkpoint (the rows of this launch)
    // ---- with a step size: re-run the forward grid from y_saved[0]; checkpoint k = start state of step k
    if (stepped) {
        for (int bl = 0; bl < nbl; ++bl) {
            float y8[8];
            row_load8(y_saved, (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, ok, 0.5f, y8);
            store8(tptr(bpY(0), bl), y8);
        }
        for (int k = 0; k < nmax && !x.aborted; ++k) {
            for (int bl = 0; bl < nbl; ++bl) {
                float y8[8];
                load8(tptr(bpY(0), bl), y8);
                row_store8(ckpt, (long long)k * ckrow + (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, ok && k < n, y8);
            }
            if (k + 1 >= nmax) break;
            const float dtl = dt_at(k);
            for (int s = 0; s < S; ++s)
                eval(IC<0>{}, bpY(s), 0, bpK(s), 0, 0, [&](int bl, float *ys, float *) { form_y(s, dtl, bl, ys); });
            for (int bl = 0; bl < nbl; ++bl) {
                float y1[8];
                advance(dtl, bl, y1);
                store8(tptr(bpY(0), bl), y1);
            }
        }
    }

    // ---- the sweep back over the grid
    for (int bl = 0; bl < nbl; ++bl) {
        float z8[8];
        zero8(z8);
        store8(tptr(bpC(), bl), z8);
    }
    int oi = T;   // outputs [oi, T) have been handed to their grid states
    for (int k = nmax - 1; k >= 0 && !x.aborted; --k) {
        const bool act = k < n;
        const double g0 = gat(k), g1 = gat(k + 1);
        const float dtl = dt_at(k);
        int lo = oi, hi = oi;
        if (act) {
            if (stepped) {
                while (lo - 1 >= 1 && sg * tb[lo - 1] > g0) --lo;   // outputs in (g_k, g_{k+1}]
            } else {
                lo = k + 1; hi = k + 2;
            }
            oi = lo;
        }
        // start state of the step; output cotangents: theta grad to grid state k + 1 (before the step's adjoint),
        // (1 - theta) grad to grid state k (after it)
        for (int bl = 0; bl < nbl; ++bl) {
            const int g8 = (blk0 + bl) * 32 + gmap(lq, 0);
            float y8[8], c8[8], p8[8];
            const long long yo = stepped ? (long long)min(k, max(n - 1, 0)) * ckrow + (long long)b * N
                                         : (long long)min(k, T - 1) * d.BN + (long long)b * N;
            row_load8(stepped ? ckpt : y_saved, yo, g8, N, ok, 0.5f, y8);
            store8(tptr(bpY(0), bl), y8);
            load8(tptr(bpC(), bl), c8);
            zero8(p8);
            for (int jo = 1; jo < T; ++jo) {
                const bool mine = act && jo >= lo && jo < hi;
                if (!__any(mine)) continue;
                const double tj = sg * tb[jo];
                float th = 1.0f;   // an output on the grid point takes that state itself
                if (mine && tj != g1)
                    th = tf32 ? ((float)tj - (float)g0) / ((float)g1 - (float)g0) : (float)((tj - g0) / (g1 - g0));
                float gv[8];
                row_load8(grad_y, (long long)jo * d.BN + (long long)b * N, g8, N, mine, 0.f, gv);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    c8[j] += th * gv[j];
                    p8[j] += (1.0f - th) * gv[j];
                }
            }
            store8(tptr(bpC(), bl), c8);
            store8(tptr(bpP(), bl), p8);
        }
        // stage inputs Y_2 .. Y_S: S - 1 plain evaluations
        for (int s = 0; s + 1 < S; ++s)
            eval(IC<0>{}, bpY(s), 0, bpK(s), 0, 0, [&](int bl, float *ys, float *) { form_y(s, dtl, bl, ys); });
        // the stages in reverse
        for (int s = S - 1; s >= 0; --s)
            eval(IC<1>{}, bpY(s), bpW(s), bpK(s), bpZ(s), s, [&](int bl, float *ys, float *ws) {
                form_y(s, dtl, bl, ys);
                form_w(s, dtl, bl, ws);
            });
        for (int bl = 0; bl < nbl; ++bl) {
            float c8[8], z8[8];
            load8(tptr(bpC(), bl), c8);
            for (int s = S - 1; s >= 0; --s) {
                load8(tptr(bpZ(s), bl), z8);
#pragma unroll
                for (int j = 0; j < 8; ++j) c8[j] += z8[j];
            }
            load8(tptr(bpP(), bl), z8);
#pragma unroll
            for (int j = 0; j < 8; ++j) c8[j] += z8[j];
            store8(tptr(bpC(), bl), c8);
        }
        if (want_grads) quadrature();
    }

    // ---- results: output 0 is y0 itself
    for (int bl = 0; bl < nbl; ++bl) {
        const int g8 = (blk0 + bl) * 32 + gmap(lq, 0);
        float c8[8], gv[8];
        load8(tptr(bpC(), bl), c8);
        row_load8(grad_y, (long long)b * N, g8, N, ok, 0.f, gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) c8[j] += gv[j];
        row_store8(adj_y0, (long long)b * N, g8, N, vb, c8);
    }
    if (gt == 0 && lq == 0 && vb) {
        status[b] = x.aborted ? (int)PHX_ERR_SYNC_TIMEOUT : st;
        nsteps_out[b] = n;
        nfe_out[b] = n * ((stepped ? 3 : 2) * S - 1);
    }
}

}  // namespace
