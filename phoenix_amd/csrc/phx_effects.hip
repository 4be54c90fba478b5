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
//                 rows of p), inside the 160 KiB of a CU; H = 40 takes 25 KiB (by LDS alone six workgroups would fit a CU; 96 VGPRs allow five waves per SIMD: an estimate, not measured).  PHX_EFFECTS has no
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
// The image, the K loops and the tile itself (efx_tile<MODE>) live in phx_effects_tile.inc, which phx_edges.hip,
// phx_netscore.hip and phx_neighbors.hip share: this unit stores the finished tile, those select from it.  The argument
// checks and the mode dispatch of the entry point are the shared ones of that file as well.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

#include "phx_effects_tile.inc"

template <int MODE>
__global__ __launch_bounds__(EFX_THREADS) void k_effects(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                         const float *__restrict__ WaT, const float *__restrict__ g,
                                                         const float *__restrict__ y, const float *__restrict__ ph,
                                                         float *__restrict__ out, int N, int H, int B, int row0, int row1)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = row0 + blockIdx.y * EFX_TILE, j0 = blockIdx.x * EFX_TILE;
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;           // this wave's corner inside the tile
    f4 v[2][2];
    efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, v);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jb = j0 + jw + 16 * tj + 4 * lq;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            const int i = i0 + iw + 16 * ti + lc;
            if (i >= row1 || jb >= N) continue;
            float *dst = out + (size_t)(i - row0) * N + jb;
            if (jb + 3 < N) {
                __builtin_memcpy(dst, &v[ti][tj], sizeof(f4));   // dword-aligned 16-byte store (rows of any N)
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (jb + r < N) dst[r] = v[ti][tj][r];
            }
        }
    }
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
    if (!efx_args_ok(p, mode, y, ph, B, 0, 0) || !out) return PHX_ERR_BAD_ARG;
    if (row0 < 0 || row1 > p->N || row0 >= row1) return PHX_ERR_BAD_ARG;
    if ((row1 - row0 + EFX_TILE - 1) / EFX_TILE > 65535) return PHX_ERR_BAD_ARG;
    const size_t need = phx_effects_workspace_bytes(p->N, p->H, B, mode);
    if (workspace_bytes < need || (need && !workspace)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    return efx_dispatch(mode, false, y, ph, B, [&](auto MODE, auto, const float *ys, const float *phs, int Bs) {
        return effects_launch<decltype(MODE)::value>(p, ys, phs, Bs, row0, row1, out, st);
    });
}

}  // extern "C"
