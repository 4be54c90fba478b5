// phx_steady_resp.hip -- the network of total effects at a fixed point (phoenix_amd.steady_state_response, DESIGN.md
// section 8r).  On the moving genes r(y) + u = 0, so (I - M Wa C) dy = M du, M = diag(m) with m = 1 on the genes that move in
// the row and 0 elsewhere, and by the Woodbury identity of section 8o
//     R = dy / du = M + M Wa Z C M,   Z = (I - S)^-1 (2H x 2H),   S = C M Wa   (phx_reduced_jacobian with this m).
// Holding gene k and moving its level gives dy / d(level k) = R[:, k] / R[k, k].
//
//   k_sr_inverse    Z_b in double: LU with partial pivoting on [I - S_b | I], one workgroup of sixteen waves per state, the
//                   steps (phx_dense_lu.inc), the pivot rule and the info codes of k_st_solve (phx_steady.hip); back
//                   substitution of the n right-hand sides a row at a time.  Every entry is updated by one thread per
//                   step, in an order fixed by n alone.
//   k_sr_factors    x_bk = Z_b C_b[:, gene k] before its scaling: a per-state contraction over the hidden index,
//                   v_mfma_f32_16x16x4_f32, a wave owns 16 rows of Z x 64 regulators; A operand Z_b[c, j] (second half:
//                   times v_bj), B operand Ws[j, gene] / Wp[j, gene] straight from the engine layout (K-major); the two
//                   halves in accumulators of their own, a' and l' applied once per (b, k) behind the contraction.
//   k_sr_scale      one thread per (b, k): d_bk = 1 + m_bk sum_c WaT[c, gene] x_bk[c], c ascending; the column times m_bk
//                   (production) or divided by d_bk (level); zeros and use = 0 where the row is left out.
//   k_sr_response   the hot kernel.  A workgroup (256 threads, four waves of 32 x 32 outputs) owns 64 regulators x 64
//                   targets in accumulators for the whole loop over the states.  It walks (state, 32 rows of the 2H) steps:
//                   the X chunk of a step lies in one half of a double buffer in LDS (the K-major panels and the K loop of
//                   phx_steady_tile.inc), the chunk of the
//                   NEXT step is requested from global memory before the products of this one and stored behind them: one
//                   barrier per step.  The WaT panel of the tile's targets does not depend on the state: it is loaded once
//                   and stays in LDS where the workgroup stays within 64 KiB (2H <= 128: two workgroups and more per CU),
//                   else its chunk travels with the X chunk.  Per state the 2H products go into a second set of
//                   accumulators, which is folded into the first as m_bj x (absolute value for mean_abs) at the state's
//                   last chunk.  The tile is stored once with plain stores: no N x N temporary, no atomics.
//   sum order       entry (k, j): per state the fmaf chain of the MFMA over c ascending (four lanes' chains of every fourth
//                   c, added by the instruction in a fixed order), then the states ascending.  A regulator's position in
//                   its tile changes no operation: a block of regulators gives the bits of the same rows of the full call.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/phoenix_hip.h"
#include "phx_device.hpp"
#include "phx_host.hpp"

namespace {

#include "phx_dense_lu.inc"
#include "phx_steady_tile.inc"

constexpr int INV_THREADS = 1024;     // threads of a workgroup of k_sr_inverse
constexpr int SR_CHUNK = TILE_KC * TILE_LDK;      // floats of a staged chunk
constexpr int SR_RES_CHUNKS = 4;      // the WaT panel stays in LDS up to this many chunks (2H <= 128)

// Z_b = (I - S_b)^-1.  A [B][n][2n] doubles of workspace: [I - S | I], eliminated in place; info[b] = 0, or k + 1 where
// column k has no finite non-zero pivot, or -1 where the inverse is not finite as float (an entry beyond the float range
// counts, as the result is stored as float); Z of such a state is zero.
__global__ __launch_bounds__(INV_THREADS) void k_sr_inverse(const float *__restrict__ S, int n, double *__restrict__ Aall,
                                                            float *__restrict__ Z, int *__restrict__ info)
{
    constexpr int NW = INV_THREADS / 64;
    __shared__ double lcol[2 * STEADY_MAX_H], rv[NW];
    __shared__ int ri[NW];
    const int b = blockIdx.x, tid = threadIdx.x, n2 = 2 * n;
    double *A = Aall + (size_t)b * n * n2;
    const float *Sb = S + (size_t)b * n * n;
    for (int idx = tid; idx < n * n2; idx += INV_THREADS) {
        const int i = idx / n2, j = idx - i * n2;
        A[idx] = j < n ? (i == j ? 1.0 : 0.0) - (double)Sb[(size_t)i * n + j] : (j - n == i ? 1.0 : 0.0);
    }
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < n; ++k) {
        int piv;
        if (!pivot<INV_THREADS>(A, n2, n, k, rv, ri, piv)) {      // a non-finite entry wins and ends the state
            bad = k + 1;
            break;
        }
        if (piv != k) swap_rows<INV_THREADS>(A, n2, k, piv, n2);
        __syncthreads();                       // the rows are swapped; rv, ri are read
        const double pv = A[(size_t)k * n2 + k];
        for (int i = k + 1 + tid; i < n; i += INV_THREADS) lcol[i] = A[(size_t)i * n2 + k] / pv;
        __syncthreads();
        eliminate<INV_THREADS>(A, n2, k, k + 1, n, k + 1, n2, lcol);      // the trailing block and the right-hand sides
        __syncthreads();
    }
    if (!bad) {
        // back substitution of the n right-hand sides (columns n .. 2n - 1), row k of the result first
        for (int k = n - 1; k >= 0; --k) {
            const double pv = A[(size_t)k * n2 + k];
            for (int j = n + tid; j < n2; j += INV_THREADS) A[(size_t)k * n2 + j] /= pv;
            for (int i = tid; i < k; i += INV_THREADS) lcol[i] = A[(size_t)i * n2 + k];
            __syncthreads();
            eliminate<INV_THREADS>(A, n2, k, 0, k, n, n2, lcol);
            __syncthreads();
        }
        int nf = 0;
        for (int idx = tid; idx < n * n; idx += INV_THREADS) {
            const int i = idx / n, j = idx - i * n;
            nf |= !finite_as_float(A[(size_t)i * n2 + n + j]);
        }
        if (__syncthreads_or(nf)) bad = -1;
    }
    float *Zb = Z + (size_t)b * n * n;
    for (int idx = tid; idx < n * n; idx += INV_THREADS) {
        const int i = idx / n, j = idx - i * n;
        Zb[idx] = bad ? 0.f : (float)A[(size_t)i * n2 + n + j];
    }
    if (tid == 0) info[b] = bad;
}

// X[b, c, k] = a'(y) sum_j Z_b[c, j] Ws[j, gene] + l'(y) sum_j (Z_b[c, H + j] v_bj) Wp[j, gene], y = y[b, gene], gene =
// genes[k]; grid (regulator tiles of 64, row tiles of 64, states); wave w: rows 16 w .. 16 w + 15 of the row tile
__global__ __launch_bounds__(ST_THREADS) void k_sr_factors(const float *__restrict__ Ws, const float *__restrict__ Wp, int N, int H,
                                                           const float *__restrict__ y, const float *__restrict__ hid,
                                                           const float *__restrict__ Z, const int *__restrict__ genes, int K,
                                                           float *__restrict__ X)
{
    // (not one of the 64 x 64 tile kernels: a wave owns 16 rows x 64 regulators, so no tile_lane)
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, H2 = 2 * H, c0 = blockIdx.y * TILE + 16 * wv, k0 = blockIdx.x * TILE;
    if (c0 >= H2) return;                      // uniform over the wave; the kernel has no barrier
    const int row = c0 + lc;
    const bool rowok = row < H2;
    const float *Zrow = Z + ((size_t)b * H2 + (rowok ? row : H2 - 1)) * H2;
    const float *vb = hid + (size_t)b * H2 + H;
    int gene[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int k = k0 + 16 * tj + lc;
        gene[tj] = k < K ? genes[k] : -1;
    }
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 as[4], ap[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) as[tj] = ap[tj] = zero;
    for (int j0 = 0; j0 < H; j0 += 4) {
        const int j = j0 + lq;
        const bool jok = j < H;
        const float zs = rowok && jok ? Zrow[j] : 0.f;
        const float zp = rowok && jok ? Zrow[H + j] * vb[j] : 0.f;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            const bool ok = jok && gene[tj] >= 0;
            const float ws = ok ? Ws[(size_t)j * N + gene[tj]] : 0.f;
            const float wp = ok ? Wp[(size_t)j * N + gene[tj]] : 0.f;
            as[tj] = mfma4(zs, ws, as[tj]);
            ap[tj] = mfma4(zp, wp, ap[tj]);
        }
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int k = k0 + 16 * tj + lc;
        if (k >= K) continue;
        float da, dl;
        phx::act_grad(y[(size_t)b * N + gene[tj]], da, dl);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + 4 * lq + r;
            if (c < H2) X[((size_t)b * H2 + c) * K + k] = fmaf(dl, ap[tj][r], da * as[tj][r]);
        }
    }
}

// one thread per (state, regulator): d = 1 + m sum_c WaT[c, gene] x[c] (c ascending), the column times m (input 0) or
// divided by d (input 1); a column that is left out -- info[b] != 0, d zero or not finite -- is zeroed, use = 0
__global__ __launch_bounds__(ST_THREADS) void k_sr_scale(const float *__restrict__ WaT, int N, int H2, const float *__restrict__ m,
                                                         const int *__restrict__ info, const int *__restrict__ genes, int K, int input,
                                                         float *__restrict__ X, float *__restrict__ use)
{
    const int b = blockIdx.y, k = blockIdx.x * ST_THREADS + threadIdx.x;
    if (k >= K) return;
    const int gene = genes[k];
    const float mv = m[(size_t)b * N + gene];
    float *col = X + (size_t)b * H2 * K + k;
    bool ok = info[b] == 0;
    float d = 1.f;
    if (ok) {
        float dot = 0.f;
        for (int c = 0; c < H2; ++c) dot = fmaf(WaT[(size_t)c * N + gene], col[(size_t)c * K], dot);
        if (mv != 0.f) d = fmaf(mv, dot, 1.f);
        else if (!finite_as_float(dot)) d = dot;       // a non-finite column of a held regulator
        ok = finite_as_float(d) && d != 0.f;
    }
    for (int c = 0; c < H2; ++c) {
        const float x = col[(size_t)c * K];
        col[(size_t)c * K] = !ok ? 0.f : (input == 0 ? (mv != 0.f ? x * mv : 0.f) : x / d);
    }
    use[(size_t)b * K + k] = ok ? 1.f : 0.f;
}

struct sr_args {
    const float *WaT, *m, *X, *use;
    const int *genes;
    float *out;
    long long ld;
    int N, H2, B, K, input, mean_abs;
};

// the chunk (state b, rows 32 t ..) of X for regulators k0 .., and of the WaT panel for targets j0 ..: two quads per thread
__device__ __forceinline__ void sr_fetch_x(const sr_args &a, int b, int t, int k0, int tid, f4 (&v)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int idx = tid + u * ST_THREADS, rr = idx >> 4, c4 = (idx & 15) * 4, c = t * TILE_KC + rr;
        const int left = a.K - (k0 + c4);
        const bool in = c < a.H2 && left > 0;
        v[u] = ld4(a.X + ((size_t)b * a.H2 + (in ? c : 0)) * a.K + (in ? k0 + c4 : 0), in ? left : 0);
    }
}

__device__ __forceinline__ f4 sr_fetch_w(const sr_args &a, int c, int j0, int c4)
{
    const int left = a.N - (j0 + c4);
    const bool in = c < a.H2 && left > 0;
    return ld4(a.WaT + (size_t)(in ? c : 0) * a.N + (in ? j0 + c4 : 0), in ? left : 0);
}

__device__ __forceinline__ void sr_store(float *buf, int tid, const f4 (&v)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int idx = tid + u * ST_THREADS, rr = idx >> 4, c4 = (idx & 15) * 4;
        *reinterpret_cast<f4 *>(buf + rr * TILE_LDK + c4) = v[u];      // 16-byte aligned
    }
}

template <bool RESIDENT>
__global__ __launch_bounds__(ST_THREADS) void k_sr_response(sr_args a)
{
    extern __shared__ __attribute__((aligned(16))) float sr_lds[];
    float *xbuf = sr_lds;                       // [2][SR_CHUNK]
    float *wbuf = sr_lds + 2 * SR_CHUNK;        // RESIDENT: [T][SR_CHUNK], else [2][SR_CHUNK]
    const tile_lane L = tile_lanes();
    const int tid = L.tid, lc = L.lc, lq = L.lq, iw = L.iw, jw = L.jw;
    const int j0 = blockIdx.x * TILE, k0 = blockIdx.y * TILE;
    const int T = (a.H2 + TILE_KC - 1) / TILE_KC, steps = a.B * T;
    const bool active = k0 + iw < a.K && j0 + jw < a.N;          // the wave has outputs inside the matrix (uniform)

    int gene[2][4];                             // the gene of the lane's rows, -1 outside
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + iw + 16 * ti + 4 * lq + r;
            gene[ti][r] = k < a.K ? a.genes[k] : -1;
        }
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 acc[2][2], dot[2][2], cnt[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        cnt[ti] = zero;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = dot[ti][tj] = zero;
    }

    f4 xv[2], wq[2];
    sr_fetch_x(a, 0, 0, k0, tid, xv);
    if (RESIDENT) {
        for (int idx = tid; idx < T * TILE_KC * 16; idx += ST_THREADS) {
            const int rr = idx >> 4, c4 = (idx & 15) * 4;
            *reinterpret_cast<f4 *>(wbuf + rr * TILE_LDK + c4) = sr_fetch_w(a, rr, j0, c4);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + u * ST_THREADS;
            wq[u] = sr_fetch_w(a, idx >> 4, j0, (idx & 15) * 4);
        }
        sr_store(wbuf, tid, wq);
    }
    sr_store(xbuf, tid, xv);
    __syncthreads();

    float mj[2] = {0.f, 0.f};
    f4 us[2] = {zero, zero};
    int b = 0, t = 0;
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        int bn = b, tn = t + 1;
        if (tn == T) {
            tn = 0;
            ++bn;
        }
        const bool more = s + 1 < steps;
        if (more) {                             // the next chunk is on its way during the products of this one
            sr_fetch_x(a, bn, tn, k0, tid, xv);
            if (!RESIDENT) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int idx = tid + u * ST_THREADS;
                    wq[u] = sr_fetch_w(a, tn * TILE_KC + (idx >> 4), j0, (idx & 15) * 4);
                }
            }
        }
        if (t == 0 && active) {                 // the state's target weights and the flags of its regulators
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const int j = j0 + jw + 16 * tj + lc;
                mj[tj] = j < a.N ? a.m[(size_t)b * a.N + j] : 0.f;
            }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) us[ti][r] = gene[ti][r] >= 0 ? a.use[(size_t)b * a.K + k0 + iw + 16 * ti + 4 * lq + r] : 0.f;
        }
        if (active) {
            const float *pa = xbuf + cur * SR_CHUNK + lq * TILE_LDK + iw + lc;
            const float *pb = (RESIDENT ? wbuf + t * SR_CHUNK : wbuf + cur * SR_CHUNK) + lq * TILE_LDK + jw + lc;
            tile_kloop<1, TILE_LDK>(pa, pb, pb, 2, 2, dot);     // an active wave computes all four tiles
            if (t == T - 1) {                   // the state is complete: fold it into the tile
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) {
                    cnt[ti] += us[ti];
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) {
                        const int j = j0 + jw + 16 * tj + lc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v = mj[tj] != 0.f ? mj[tj] * dot[ti][tj][r] : 0.f;
                            if (gene[ti][r] == j) v = a.input == 0 ? v + mj[tj] * us[ti][r] : 0.f;
                            acc[ti][tj][r] += a.mean_abs ? fabsf(v) : v;
                        }
                        dot[ti][tj] = zero;
                    }
                }
            }
        }
        if (more) {
            sr_store(xbuf + (cur ^ 1) * SR_CHUNK, tid, xv);
            if (!RESIDENT) sr_store(wbuf + (cur ^ 1) * SR_CHUNK, tid, wq);
        }
        __syncthreads();
        b = bn;
        t = tn;
    }

    if (!active) return;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + iw + 16 * ti + 4 * lq + r;
            if (k >= a.K) continue;
            const float n = cnt[ti][r];
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const int j = j0 + jw + 16 * tj + lc;
                if (j >= a.N) continue;
                float v = acc[ti][tj][r] / (n > 0.f ? n : 1.f);
                if (a.input == 1 && gene[ti][r] == j) v = n > 0.f ? 1.f : 0.f;
                a.out[(size_t)k * a.ld + j] = v;
            }
        }
}

}  // namespace

extern "C" {

size_t phx_steady_inverse_workspace_bytes(int H, int B)
{
    if (!steady_shape_ok(/* N */ 1, H, B)) return 0;
    return (size_t)B * 8 * H * H * sizeof(double);
}

int phx_steady_inverse(const float *S, int H, int B, float *Z, int *info, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!S || !Z || !info || !steady_shape_ok(/* N */ 1, H, B)) return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_steady_inverse_workspace_bytes(H, B)) return PHX_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_sr_inverse, dim3((unsigned)B), dim3(INV_THREADS), 0, (hipStream_t)stream, S, 2 * H,
                       static_cast<double *>(workspace), Z, info);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

int phx_steady_response_factors(const phx_params *p, const float *y, const float *m, const float *hid, const float *Z,
                                const int *info, int B, const int *genes, int K, int input, float *X, float *use, void *stream)
{
    if (!steady_shape_ok(p, B) || !p->Ws || !p->Wp || !p->WaT || !y || !m || !hid || !Z || !info || !genes || !X || !use)
        return PHX_ERR_BAD_ARG;
    if (B > 65535 || K < 1 || (input != 0 && input != 1)) return PHX_ERR_BAD_ARG;
    const int N = p->N, H = p->H, H2 = 2 * H;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sr_factors, dim3((unsigned)((K + TILE - 1) / TILE), (unsigned)((H2 + TILE - 1) / TILE), (unsigned)B),
                       dim3(ST_THREADS), 0, st, p->Ws, p->Wp, N, H, y, hid, Z, genes, K, X);
    if (!launched()) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL(k_sr_scale, dim3((unsigned)((K + ST_THREADS - 1) / ST_THREADS), (unsigned)B), dim3(ST_THREADS), 0, st, p->WaT,
                       N, H2, m, info, genes, K, input, X, use);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

int phx_steady_response(const phx_params *p, const float *m, const float *X, const float *use, int B, const int *genes, int K,
                        int input, int mean_abs, float *out, long long ld, void *stream)
{
    if (!steady_shape_ok(p, B) || !p->WaT || !m || !X || !use || !genes || !out) return PHX_ERR_BAD_ARG;
    if (K < 1 || (input != 0 && input != 1) || ld < p->N) return PHX_ERR_BAD_ARG;
    const int H2 = 2 * p->H, T = (H2 + TILE_KC - 1) / TILE_KC;
    if ((long long)B * T > 0x7fffffffLL) return PHX_ERR_BAD_ARG;
    sr_args a;
    a.WaT = p->WaT;
    a.m = m;
    a.X = X;
    a.use = use;
    a.genes = genes;
    a.out = out;
    a.ld = ld;
    a.N = p->N;
    a.H2 = H2;
    a.B = B;
    a.K = K;
    a.input = input;
    a.mean_abs = mean_abs != 0;
    const dim3 grid((unsigned)((p->N + TILE - 1) / TILE), (unsigned)((K + TILE - 1) / TILE));
    if (T <= SR_RES_CHUNKS)
        hipLaunchKernelGGL(k_sr_response<true>, grid, dim3(ST_THREADS), (size_t)(2 + T) * SR_CHUNK * sizeof(float),
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_sr_response<false>, grid, dim3(ST_THREADS), (size_t)4 * SR_CHUNK * sizeof(float), (hipStream_t)stream, a);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // extern "C"
