// phx_effects.hip -- the gene-by-gene "effects matrix" of a trained model (extract_model_matrix_PHOENIX.py:46-58) and the
// Jacobian of the RHS (odenet.py:85-91) averaged over a batch of expression states, regulator i -> target j, straight
// from the engine layout of the parameters (Ws, Wp [H, N], WaT [2H, N]: both operands of every product are K-major as
// they are, nothing is transposed or copied).  With s = y - 0.5, r = relu(g):
//     S[i,j]   = sum_h Ws[h,i] WaT[h,j]                                  (state independent)
//     Q_b[i,j] = sum_h p[b,h] Wp[h,i] WaT[H+h,j]                         p[b,:] = exp(Wp log1p(softsign(y_b)) + bp)
//     J_b[i,j] = d f_j / d y_i (y_b) = r_j ( a'(y_bi) S[i,j] + l'(y_bi) Q_b[i,j] - delta_ij )
//     effects[i,j] = r_j ( S[i,j] + sum_h Wp[h,i] WaT[H+h,j] )
// One launch of k_effects<MODE>; grid (ceil(N / 64) target tiles, ceil(rows / 64) regulator tiles), four waves per
// workgroup, a wave owns 32 x 32 entries as 2 x 2 tiles of v_mfma_f32_16x16x4_f32.
//
//   MFMA layout   The product is formed transposed, D[jj][ii] = sum_k A[jj][k] B[k][ii] with A = the WaT panel and B = the
//                 Ws / Wp panel, so that the four accumulator registers of a lane (rows 4 q .. 4 q + 3 of D, q = lane >> 4)
//                 are four consecutive targets j of ONE regulator row i (column lane & 15 of D): the result leaves in
//                 16-byte stores, 64 bytes per row and tile, and the per-regulator factors a', l' are one value per lane
//                 and tile.
//   LDS           One image of Hp = 4 ceil(H / 4) rows of EFX_LD = 144 floats: 64 regulator columns of Ws (or Wp), 64 target
//                 columns of the matching half of WaT, 16 floats of padding (rows 16 banks apart: the four k of an MFMA
//                 operand read conflict-free).  The contraction over the 2H hidden rows runs in two K chunks through the
//                 SAME image -- first [Ws ; WaT[0:H]], then [Wp ; WaT[H:2H]] -- so H = 256 takes 144 KiB (+ 2 KiB for two
//                 rows of p), inside the 160 KiB of a CU; H = 40 takes 25 KiB (by LDS alone six workgroups would fit a CU; 92 VGPRs allow five waves per SIMD: an estimate, not measured).  PHX_EFFECTS has no
//                 state loop to keep an image for: it walks both halves 32 rows at a time through an 18 KiB image.
//   state loop    S is accumulated once and stays in registers.  The second image stays in LDS for the whole state loop:
//                 per state only Q_b is recomputed (the factor p[b,h] multiplies the Wp operand on its way into the MFMA),
//                 combined with a' and l' of the lane's regulators (closed forms of y), made
//                 absolute where asked and added to the running sum -- B rank-H products per tile with the tile on chip.
//                 The row of p for the next state is written to the idle half of a two-row LDS buffer: one barrier per
//                 state.
//   out           written exactly once; no N x N temporary exists anywhere.
// Every entry is one lane's chain of fused multiply-adds over k = 0 .. Hp - 1 in that order (padding rows are zeros) and,
// in the Jacobian modes, over b = 0 .. B - 1 in that order: its bits depend on (N, H, B, mode, i, j) alone, not on the row
// range or the tile it falls into.  No atomics.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

constexpr int EFX_TILE = 64;       // regulators and targets of a workgroup
constexpr int EFX_LD = 144;        // floats of an LDS row: 64 regulator columns | 64 target columns | 16 padding
constexpr int EFX_THREADS = 256;   // four waves, 32 x 32 entries each
constexpr int EFX_MAX_H = 256;
constexpr int EFX_LDS_TAIL = 2 * EFX_MAX_H;   // two rows of p
constexpr int EFX_KC = 32;                  // hidden rows of an image of the effects mode (18 KiB)
constexpr int EFX_KU = 4;                   // K steps (of four hidden rows) whose operand reads are issued together
static_assert(EFX_MAX_H == EFX_THREADS, "thread t stages p[b, t]");

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// relu as torch computes it: a NaN multiplier stays NaN (fmaxf would turn it into 0)
__device__ __forceinline__ float efx_relu(float g) { return g > 0.f ? g : (g == g ? 0.f : g); }

// derivatives of SoftsignMod and LogShiftedSoftSignMod (odenet.py:21-35) in closed form, as phx_device.hpp: act_grad
__device__ __forceinline__ void efx_act_grad(float y, float &da, float &dl)
{
    const float s = y - 0.5f;
    const float d = 1.0f + fabsf(s);
    da = 1.0f / (d * d);
    dl = (s < 0.0f) ? 1.0f / d : 1.0f / ((1.0f + s) * (1.0f + 2.0f * s));
}

// image rows 0 .. rows - 1 = rows k0 .. of wi [H, N] (columns i0 .. i0 + 63) and of wj [H, N] (columns j0 .. j0 + 63), a
// quad of columns per thread and step (dword-aligned 16-byte loads, one ds_write_b128); zeros outside the matrices
__device__ __forceinline__ void efx_stage(float *img, const float *__restrict__ wi, const float *__restrict__ wj, int i0, int j0,
                                          int N, int H, int k0, int rows)
{
    for (int idx = threadIdx.x; idx < rows * (2 * EFX_TILE / 4); idx += EFX_THREADS) {
        const int kr = idx >> 5, c = (idx & 31) * 4, k = k0 + kr;
        const int col = c < EFX_TILE ? i0 + c : j0 + c - EFX_TILE;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < H && col < N) {
            const float *src = (c < EFX_TILE ? wi : wj) + (size_t)k * N + col;
            if (col + 3 < N) {
                __builtin_memcpy(&v, src, sizeof(f4));
            } else {
                v[0] = src[0];
                if (col + 1 < N) v[1] = src[1];
                if (col + 2 < N) v[2] = src[2];
            }
        }
        *reinterpret_cast<f4 *>(img + kr * EFX_LD + c) = v;
    }
}

// acc[ti][tj] += sum over the image's rows of  B(regulator tile ti) * A(target tile tj);  SCALE: row k of the regulator
// panel is multiplied by pp[k] first (pa, pb, pp already point at this lane's k = lane >> 4)
// one step: four k (this lane holds k = lane >> 4 of them)
template <bool SCALE>
__device__ __forceinline__ void efx_kstep(float a0, float a1, float b0, float b1, float s, f4 (&acc)[2][2])
{
    if (SCALE) {
        b0 *= s;
        b1 *= s;
    }
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a1, b0, acc[0][1]);
    acc[1][0] = mfma4(a0, b1, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
}

template <bool SCALE>
__device__ __forceinline__ void efx_kloop(const float *pa, const float *pb, const float *pp, int nk, f4 (&acc)[2][2])
{
    // four steps at a time: their 16 operand reads are issued together and the 16 MFMAs wait for them one step after the
    // other, so the LDS latency is paid once per group even with one wave per SIMD (k ascends as in the plain loop)
    int kk = 0;
    for (; kk + EFX_KU <= nk; kk += EFX_KU) {
        float a0[EFX_KU], a1[EFX_KU], b0[EFX_KU], b1[EFX_KU], s[EFX_KU];
#pragma unroll
        for (int u = 0; u < EFX_KU; ++u) {
            a0[u] = pa[4 * u * EFX_LD];
            a1[u] = pa[4 * u * EFX_LD + 16];
            b0[u] = pb[4 * u * EFX_LD];
            b1[u] = pb[4 * u * EFX_LD + 16];
            s[u] = SCALE ? pp[4 * u] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < EFX_KU; ++u) efx_kstep<SCALE>(a0[u], a1[u], b0[u], b1[u], s[u], acc);
        pa += 4 * EFX_KU * EFX_LD;
        pb += 4 * EFX_KU * EFX_LD;
        if (SCALE) pp += 4 * EFX_KU;
    }
    for (; kk < nk; ++kk) {
        efx_kstep<SCALE>(pa[0], pa[16], pb[0], pb[16], SCALE ? pp[0] : 1.f, acc);
        pa += 4 * EFX_LD;
        pb += 4 * EFX_LD;
        if (SCALE) pp += 4;
    }
}

template <int MODE>
__global__ __launch_bounds__(EFX_THREADS) void k_effects(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                         const float *__restrict__ WaT, const float *__restrict__ g,
                                                         const float *__restrict__ y, const float *__restrict__ ph,
                                                         float *__restrict__ out, int N, int H, int B, int row0, int row1)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hp = (H + 3) & ~3, nk = Hp >> 2;
    float *img = lds, *phs = lds + Hp * EFX_LD;                  // phs [2][EFX_MAX_H]
    const int i0 = row0 + blockIdx.y * EFX_TILE, j0 = blockIdx.x * EFX_TILE;
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;           // this wave's corner inside the tile
    const float *pb = img + lq * EFX_LD + iw + lc;               // regulator panel, B operand
    const float *pa = img + lq * EFX_LD + EFX_TILE + jw + lc;    // target panel, A operand
    const f4 zero = {0.f, 0.f, 0.f, 0.f};

    f4 S[2][2] = {{zero, zero}, {zero, zero}};
    f4 acc[2][2] = {{zero, zero}, {zero, zero}};
    if (MODE == PHX_EFFECTS) {
        // one accumulator over [Ws ; WaT[0:H]] and then [Wp ; WaT[H:2H]], EFX_KC rows at a time: the image is small, so
        // several workgroups share a CU (eight by LDS and the wave limit: an estimate) and the staging of one can run
        // under the MFMAs of the others
        for (int half = 0; half < 2; ++half) {
            const float *wi = half ? Wp : Ws, *wj = WaT + (size_t)half * H * N;
            for (int k0 = 0; k0 < Hp; k0 += EFX_KC) {
                const int rows = min(EFX_KC, Hp - k0);
                __syncthreads();                                 // every wave is done with the previous rows
                efx_stage(img, wi, wj, i0, j0, N, H, k0, rows);
                __syncthreads();
                efx_kloop<false>(pa, pb, nullptr, rows >> 2, acc);
            }
        }
    } else {
        efx_stage(img, Ws, WaT, i0, j0, N, H, 0, Hp);
        __syncthreads();
        efx_kloop<false>(pa, pb, nullptr, nk, S);
        __syncthreads();                                         // every wave is done with the first image
        efx_stage(img, Wp, WaT + (size_t)H * N, i0, j0, N, H, 0, Hp);
        phs[tid] = tid < H ? ph[tid] : 0.f;
        __syncthreads();
        int ig[2];                                               // this lane's two regulators
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) ig[ti] = i0 + iw + 16 * ti + lc;
        float yn[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) yn[ti] = ig[ti] < N ? y[ig[ti]] : 0.5f;
        for (int b = 0; b < B; ++b) {
            // what state b + 1 needs from memory is asked for now and used after this state's products
            const float pn = (b + 1 < B && tid < H) ? ph[(size_t)(b + 1) * H + tid] : 0.f;
            float yv[2];
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                yv[ti] = yn[ti];
                if (b + 1 < B && ig[ti] < N) yn[ti] = y[(size_t)(b + 1) * N + ig[ti]];
            }
            f4 Q[2][2] = {{zero, zero}, {zero, zero}};
            efx_kloop<true>(pa, pb, phs + (b & 1) * EFX_MAX_H + lq, nk, Q);
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                float da, dl;
                efx_act_grad(yv[ti], da, dl);
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const int jb = j0 + jw + 16 * tj + 4 * lq;   // first of this lane's four targets
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = fmaf(dl, Q[ti][tj][r], da * S[ti][tj][r]);
                        if (ig[ti] == jb + r) v -= 1.0f;
                        acc[ti][tj][r] += MODE == PHX_JAC_MEAN_ABS ? fabsf(v) : v;
                    }
                }
            }
            phs[((b + 1) & 1) * EFX_MAX_H + tid] = pn;
            __syncthreads();                                     // p of state b is read, p of state b + 1 is written
        }
    }

    const float fB = (float)B;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jb = j0 + jw + 16 * tj + 4 * lq;
        f4 rj;
#pragma unroll
        for (int r = 0; r < 4; ++r) rj[r] = jb + r < N ? efx_relu(g[jb + r]) : 0.f;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            const int i = i0 + iw + 16 * ti + lc;
            f4 v = acc[ti][tj];
            if (MODE != PHX_EFFECTS) v = v / fB;                 // the mean first: a sum of B ones leaves as exactly 1
            v = v * rj;
            if (i >= row1 || jb >= N) continue;
            float *dst = out + (size_t)(i - row0) * N + jb;
            if (jb + 3 < N) {
                __builtin_memcpy(dst, &v, sizeof(f4));           // dword-aligned 16-byte store (rows of any N)
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (jb + r < N) dst[r] = v[r];
            }
        }
    }
}

bool effects_shape_ok(int N, int H) { return N >= 2 && H >= 1 && H <= EFX_MAX_H; }

size_t effects_lds_bytes(int H, int mode)
{
    const int Hp = (H + 3) & ~3;
    if (mode == PHX_EFFECTS) return (size_t)(Hp < EFX_KC ? Hp : EFX_KC) * EFX_LD * sizeof(float);
    return ((size_t)Hp * EFX_LD + EFX_LDS_TAIL) * sizeof(float);
}

template <int MODE>
int effects_launch(const phx_params *p, const float *y, const float *ph, int B, int row0, int row1, float *out,
                   hipStream_t st)
{
    const size_t lds = effects_lds_bytes(p->H, MODE);
    if (!phxh::set_lds(k_effects<MODE>, lds)) return PHX_ERR_LAUNCH;
    const dim3 grid((p->N + EFX_TILE - 1) / EFX_TILE, (row1 - row0 + EFX_TILE - 1) / EFX_TILE);
    hipLaunchKernelGGL(k_effects<MODE>, grid, dim3(EFX_THREADS), lds, st, p->Ws, p->Wp, p->WaT, p->g, y, ph, out, p->N, p->H,
                       B, row0, row1);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t phx_effects_workspace_bytes(int N, int H, int B, int mode)
{
    // the tile lives in registers and the operands in LDS: no shape needs device scratch today, so a refused shape and a
    // served one both answer 0 (and phx_effects_matrix never returns PHX_ERR_WORKSPACE); the first shape that needs
    // scratch must answer 0 for !effects_shape_ok(N, H), B < 1 in a Jacobian mode and an unknown mode
    (void)N; (void)H; (void)B; (void)mode;
    return 0;
}

int phx_effects_matrix(const phx_params *p, int mode, const float *y, const float *ph, int B, int row0, int row1, float *out,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (!p || !out || !p->Ws || !p->Wp || !p->WaT || !p->g || !effects_shape_ok(p->N, p->H)) return PHX_ERR_BAD_ARG;
    if (row0 < 0 || row1 > p->N || row0 >= row1) return PHX_ERR_BAD_ARG;
    if (mode != PHX_EFFECTS && mode != PHX_JAC_MEAN && mode != PHX_JAC_MEAN_ABS) return PHX_ERR_BAD_ARG;
    if (mode != PHX_EFFECTS && (!y || !ph || B < 1)) return PHX_ERR_BAD_ARG;
    if ((row1 - row0 + EFX_TILE - 1) / EFX_TILE > 65535) return PHX_ERR_BAD_ARG;
    const size_t need = phx_effects_workspace_bytes(p->N, p->H, B, mode);
    if (workspace_bytes < need || (need && !workspace)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    switch (mode) {
    case PHX_EFFECTS: return effects_launch<PHX_EFFECTS>(p, nullptr, nullptr, 1, row0, row1, out, st);
    case PHX_JAC_MEAN: return effects_launch<PHX_JAC_MEAN>(p, y, ph, B, row0, row1, out, st);
    default: return effects_launch<PHX_JAC_MEAN_ABS>(p, y, ph, B, row0, row1, out, st);
    }
}

}  // extern "C"
