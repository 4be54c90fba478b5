// phx_mfma_adj3_tail.inc -- k3_tail_adj3: what follows the backward solve k1_solve_adj3 (phx_mfma_adj3.inc) in place of
// k3_reduce_grads.  One ordinary launch (no polling, no flags waited on: every input was written by the solve launch in
// front of it) that
//   * for every batch group that DEFERRED the visit of its last step (header word XH_DEFER + grp, phx_mfma_v3common.inc)
//     runs that visit -- quadrature of the parameter gradient over the seven stages, dense output, jump, adj_y0 -- from
//     the group's private tiles (W1::scratch), the transposed hidden rows of its ring slots (W1::hq) and the records the
//     group left in the head of its partial;
//   * for every other group adds the partial the group wrote in the solve, as k3_reduce_grads did;
//   * writes the sum over all groups straight into the caller's gradients (phx_grads; reference layout of Wa included).
//
// Partition: a workgroup of four waves per (gene block, gene half) -- 698 at the breast-cancer shape, on all CUs where the
// solve's 236 workgroups of one wave per SIMD each ran 12 such items per wave inside a 512-register budget.  Wave w runs
// the trajectory tiles w, w + 4, ... of ALL deferred groups (tile index = group * ntg + tile of the group) through the
// same 4 HT accumulators, so a gradient element's contraction runs over the trajectories of every group inside the
// workgroup; the four waves' accumulators are added through LDS in wave order, then the partials of the groups that did
// not defer in group order: a fixed order, the same bits on every call.
//
// The visit's body is quad_accept's (phx_mfma_adj3.inc) for one (tile, half block), kept as a copy: the solve kernel's
// schedule moves with every edit of its source, and here the controller values come from the group's records instead of
// the solve's LDS.  Three more differences: the hidden rows are single buffered (the next stage's are requested behind
// the MFMAs that read the current ones; a second workgroup per CU covers the wait, which the solve kernel's one wave per
// SIMD could not), the bias gradients use the du / dv rows the MFMAs were fed with instead of loading them again, and
// 1 / relu(g) multiplies the gene-multiplier sum once at the end instead of every term.
namespace {

template <int HT>
__global__ __launch_bounds__(256, 2) void k3_tail_adj3(D1 d, W1 w, const float *__restrict__ gmul,
                                                       const float *__restrict__ grad_y, float *adj_y0, long long PP, float *gWs, float *gWp, float *gWaT,
                                                       float *gg, float *gbs, float *gbp, int overwrite, float *gWa)
{
    constexpr int F4 = 4 * HT, F2 = 2 * HT;
    __shared__ float4 red[4][F4][64];                                  // the waves' accumulators
    __shared__ __attribute__((aligned(16))) float ctl[4][16 * TR_N];   // per wave: the records of the tile it works on
    __shared__ float dgred[4][16], bred[4][2][HT * 16];
    __shared__ int sdef[256];                                          // group deferred? (TG <= 256: the header's limit)
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = blockIdx.x, gb = item >> 1, s2 = item & 1;
    const int gtile = gb / d.NB, bl = gb % d.NB;
    const int N = d.N, H = d.H, B = d.B, Bt = d.Bt, ntg = d.ntg, TG = d.TG, G = d.G;
    const bool bias_item = item == 0;   // the gene-independent dbs / dbp come from one item
    unsigned int *hdr = reinterpret_cast<unsigned int *>(w.cnt);
    for (int i = tid; i < 256; i += blockDim.x) sdef[i] = (i < TG && hdr[XH_DEFER + i] == 1u) ? 1 : 0;
    __syncthreads();

    const int tiles_wg = ntg * d.NB;
    const int lane32h = lane * 32 + 16 * s2, lane16 = lane * 16;
    const int gene0 = gb * 32;
    const long long og = (long long)d.nblk * (F4 * 2 * 256), obs = og + N, obp = obs + H;
    const __amdgpu_buffer_rsrc_t hrs = make_rsrc(w.hq, (unsigned int)((size_t)TG * ntg * 7 * F4 * 1024));
    auto ring = [&](int kb, int j) -> int { const int v = kb + j; return v >= 7 ? v - 7 : v; };
    float rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gene = gene0 + gmap(lq, 4 * s2 + j);
        const float gm = gene < N ? gmul[gene] : 0.f;
        rr[j] = gm > 0.f ? gm : 0.f;   // relu(gene_multipliers), as the LDS images hold it
    }
    f32x4 gs_[HT], gp_[HT], ga_[F2];
    float dgacc[4], sbias[HT], pbias[HT];
#pragma unroll
    for (int f = 0; f < HT; ++f) { gs_[f] = (f32x4){0.f, 0.f, 0.f, 0.f}; gp_[f] = gs_[f]; sbias[f] = 0.f; pbias[f] = 0.f; }
#pragma unroll
    for (int f = 0; f < F2; ++f) ga_[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) dgacc[j] = 0.f;

    for (int tt = wv; tt < TG * ntg; tt += 4) {
        const int grp = tt / ntg, ttl = tt % ntg;
        if (!sdef[grp]) continue;
        const float *blk = w.dtheta + (long long)grp * PP;
        // the tile's 16 records -> this wave's LDS slot (only this wave touches it: in-order LDS, no barrier)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        reinterpret_cast<float4 *>(ctl[wv])[lane] = reinterpret_cast<const float4 *>(blk + (long long)ttl * 16 * TR_N)[lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int kb = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(blk + (long long)Bt * TR_N)[ttl]);
        const float *rec = ctl[wv] + li * TR_N;
        const int b = grp * Bt + ttl * 16 + li;
        const bool okb = b < B;
        const __amdgpu_buffer_rsrc_t trs = make_rsrc(w.scratch + (long long)(grp * G + gtile) * d.nvec * tiles_wg * 512,
                                                     (unsigned int)(d.nvec * tiles_wg * 2048));
        auto toff = [&](int v) -> int { return ((v * tiles_wg) + (ttl * d.NB + bl)) * 2048; };
        auto hoff = [&](int slot, int f) -> int { return (((grp * ntg + ttl) * 7 + slot) * F4 + f) * 1024; };
        float y0v[4], a0v[4], ky[7][4], ka[7][4];
        bload4(trs, lane32h, toff(C_Y0), y0v);
        bload4(trs, lane32h, toff(C_A0), a0v);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            bload4(trs, lane32h, toff(C_KY + ring(kb, j)), ky[j]);
            bload4(trs, lane32h, toff(C_KA + ring(kb, j)), ka[j]);
        }
        // (the stage weights and the dense-output fraction stay in the LDS records until they are used)
        const float dts = rec[TR_DT], sg = rec[TR_SG];
        auto weighted = [&](int S) -> bool { return __any(rec[TR_W + S] != 0.f) != 0; };   // wave uniform
        // transposed hidden rows of a stage (du | dv first: they are used first); a stage without weight loads none
        float h[F4][4];
        auto issue_h = [&](int S) {
            const int hs = ring(kb, S);
#pragma unroll
            for (int f = 0; f < F4; ++f) bload4(hrs, lane16, hoff(hs, (f + F2) % F4), h[f]);
        };
        if (weighted(0)) issue_h(0);
        float a1[4];
        auto stage = [&](auto Sc) {
            constexpr int S = decltype(Sc)::value;
            asm volatile("; PHXMARK tail stage %0" ::"n"(S));
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
                for (int j = 0; j < 4; ++j) a1[j] = as[j];
            }
            if (weighted(S)) {
                const float wl = rec[TR_W + S];
                float w4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) w4[r] = ctl[wv][(4 * lq + r) * TR_N + TR_W + S];
                float an[4], ln[4], qn[4];
                // no masks: padding genes hold (0.5, 0) with relu(g) = 0, padding trajectories have weight zero
                act_pair_fast_pk<2>(ys, an, ln);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    qn[j] = as[j] * rr[j];
                    // a (j - y) from k_y = -sgn relu(g) (j - y)
                    // (1 / relu(g) is the same for every stage and trajectory: it multiplies the sum, below)
                    dgacc[j] += wl * (as[j] * (-sg * ky[S][j]));
                }
                float at[4], lt[4], qt[4];
                xpose4(an, at, lane);
                xpose4(ln, lt, lane);
                xpose4(qn, qt, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) { at[r] *= w4[r]; lt[r] *= w4[r]; qt[r] *= w4[r]; }
                // h[0 .. F2) = du | dv rows, h[F2 .. F4) = z_u | z_p rows: lane (li, lq), component r <-> hidden row
                // 16 f + rho16(li >> 2, li & 3) of trajectory 4 lq + r
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
                if (bias_item) {   // dbs += w du, dbp += w dv
#pragma unroll
                    for (int f = 0; f < HT; ++f) {
                        sbias[f] += ((w4[0] * h[f][0] + w4[1] * h[f][1]) + w4[2] * h[f][2]) + w4[3] * h[f][3];
                        pbias[f] += ((w4[0] * h[HT + f][0] + w4[1] * h[HT + f][1]) + w4[2] * h[HT + f][2]) + w4[3] * h[HT + f][3];
                    }
                }
            }
            // the next weighted stage's rows, behind the MFMAs that read this stage's
            __builtin_amdgcn_sched_barrier(0);
            if (S < 6 && weighted(S < 6 ? S + 1 : 6)) issue_h(S + 1);
        };
        stage(I3<0>{}); stage(I3<1>{}); stage(I3<2>{}); stage(I3<3>{}); stage(I3<4>{}); stage(I3<5>{});
        const bool adv = rec[TR_ADV] != 0.f;
        float gy4[4];
        {   // jump data at t_0 (adjoint.py:152-154: a deferred visit is the one that reaches the first time point)
            const long long ro = (long long)b * N;
            const int g0 = gene0 + gmap(lq, 4 * s2);
            row_load4(grad_y, ro, g0, N, okb && adv, 0.f, gy4);
        }
        stage(I3<6>{});
        asm volatile("; PHXMARK tail accept");
        // ---- accept pass (rk_common.py:168-196; dense output interp.py:1-47; jump adjoint.py:152-154) -> adj_y0
        {
            float am[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) am[j] = ka[0][j] * (dts * DP_CMID[0]);
#pragma unroll
            for (int kk = 2; kk < 6; ++kk) {   // DP_CMID[1] == 0
                const float cf = dts * DP_CMID[kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) am[j] += ka[kk][j] * cf;
            }
            const InterpX ix = {rec[TR_X], rec[TR_X + 1], rec[TR_X + 2], rec[TR_X + 3]};
            float anew[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                am[j] += ka[6][j] * (dts * DP_CMID[6]);
                const float aout = interp_eval(a0v[j], a1[j], a0v[j] + am[j], ka[0][j], ka[6][j], dts, ix);
                anew[j] = adv ? aout + gy4[j] : a0v[j];   // (a trajectory that was out before the step keeps its state)
            }
            row_store4(adj_y0, (long long)b * N, gene0 + gmap(lq, 4 * s2), N, okb, anew);
        }
    }

    // ---- the four waves' sums -> LDS
#pragma unroll
    for (int f = 0; f < HT; ++f) {
        red[wv][0 * HT + f][lane] = make_float4(gs_[f][0], gs_[f][1], gs_[f][2], gs_[f][3]);
        red[wv][1 * HT + f][lane] = make_float4(gp_[f][0], gp_[f][1], gp_[f][2], gp_[f][3]);
        red[wv][2 * HT + f][lane] = make_float4(ga_[f][0], ga_[f][1], ga_[f][2], ga_[f][3]);
        red[wv][3 * HT + f][lane] = make_float4(ga_[HT + f][0], ga_[HT + f][1], ga_[HT + f][2], ga_[HT + f][3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // dg: sum over the trajectories of a tile position (lanes with equal lq)
        // a (j - y) from k_y = -sgn relu(g) (j - y): exactly 0 where relu(g) = 0
        float v = rr[j] > 0.f ? dgacc[j] * fast_rcp(rr[j]) : 0.f;
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
        if (li == 0) dgred[wv][lq * 4 + j] = v;
    }
    if (bias_item) {
#pragma unroll
        for (int f = 0; f < HT; ++f) {
            float sb = sbias[f], sp = pbias[f];
            sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
            sp += __shfl_xor(sp, 16, 64); sp += __shfl_xor(sp, 32, 64);
            if (lq == 0) { bred[wv][0][f * 16 + li] = sb; bred[wv][1][f * 16 + li] = sp; }
        }
    }
    __syncthreads();

    // ---- wave w finishes accumulators w, w + 4, ...: waves in order, then the partials of the groups that did not defer
    // (accumulator-native order, see k1_solve_adj3) in group order, then out as k3_reduce_grads writes them
    for (int mf = wv; mf < F4; mf += 4) {
        float4 sacc = red[0][mf][lane];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float4 v = red[k][mf][lane];
            sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
        }
        const long long slot = ((long long)gb * (F4 * 2) + mf * 2 + s2) * 64 + lane;
        for (int g = 0; g < TG; ++g)
            if (!sdef[g]) {
                const float4 v = reinterpret_cast<const float4 *>(w.dtheta + (long long)g * PP)[slot];
                sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
            }
        const int m = mf / HT, f = mf % HT;
        const int gene = gene0 + gmapC(li, s2);
        float *dst = (m == 0) ? gWs : (m == 1 ? gWp : (m == 2 ? gWaT : gWaT + (long long)H * N));
        const float o[4] = {sacc.x, sacc.y, sacc.z, sacc.w};
        if (gene >= N) continue;
        if (gWa && m >= 2) {   // reference layout [N, 2H] (phx_grads.Wa)
            float *q = gWa + (long long)gene * 2 * H + (m - 2) * H + 16 * f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rw = rho16(lq, r);
                if (16 * f + rw < H) q[rw] = overwrite ? o[r] : q[rw] + o[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * f + rho16(lq, r);
                if (row < H) {
                    float *q = dst + (long long)row * N + gene;
                    *q = overwrite ? o[r] : *q + o[r];
                }
            }
        }
    }
    if (tid < 16) {   // dg of the lane group's gene (tid = 4 lq + j)
        const int gene = gene0 + gmap(tid >> 2, 4 * s2 + (tid & 3));
        if (gene < N) {
            float v = ((dgred[0][tid] + dgred[1][tid]) + dgred[2][tid]) + dgred[3][tid];
            for (int g = 0; g < TG; ++g)
                if (!sdef[g]) v += w.dtheta[(long long)g * PP + og + gene];
            gg[gene] = overwrite ? v : gg[gene] + v;
        }
    }
    if (bias_item && tid >= 64 && tid < 64 + HT * 16) {
        const int e = tid - 64, f = e >> 4, i = e & 15;
        const int hid = 16 * f + rho16(i >> 2, i & 3);   // the transposed rows' lane i holds this hidden row
        if (hid < H) {
            float sb = ((bred[0][0][e] + bred[1][0][e]) + bred[2][0][e]) + bred[3][0][e];
            float sp = ((bred[0][1][e] + bred[1][1][e]) + bred[2][1][e]) + bred[3][1][e];
            for (int g = 0; g < TG; ++g)
                if (!sdef[g]) { sb += w.dtheta[(long long)g * PP + obs + hid]; sp += w.dtheta[(long long)g * PP + obp + hid]; }
            gbs[hid] = overwrite ? sb : gbs[hid] + sb;
            gbp[hid] = overwrite ? sp : gbp[hid] + sp;
        }
    }
    if (bias_item && tid == 0) {
        int n = 0;
        for (int g = 0; g < TG; ++g) n += sdef[g];
        hdr[XH_SERVED] = (unsigned int)n;
    }
}

}  // namespace
