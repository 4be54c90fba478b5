// phx_netscore.hip -- scoring the matrices of phx_effects.hip against a known network without the matrices: the two
// device passes behind `effects_at` and `network_score` (network-recovery AUROC / average precision), both epilogues of
// the 64 x 64 MFMA tile engine (phx_effects_tile.inc) that phx_effects_matrix stores and phx_effects_edges selects from.
// Every tile is recomputed in each pass; every value has the bits phx_effects_matrix writes for that entry.
// The SCORE of entry (i, j) is its magnitude bits m = bits & 0x7fffffff.  With PHX_EDGES_ORIENT the scored matrix is
// make_mask (extract_model_matrix_PHOENIX.py:29-37) of M: an entry keeps its value only when |M[i,j]| > |M[j,i]| as
// floats (a NaN on either side fails the comparison), every other entry and the diagonal are +0.
//
//   tiles         As k_edges: without ORIENT a workgroup owns tile (I, J); with ORIENT the unordered pair I <= J, forms
//                 both tiles and decides both directions of every gene pair once (efx_tile_of_block, efx_park and
//                 efx_tile_pair of phx_effects_tile.inc).
//   GATHER pass   keys[n] = i N + j grouped by tile (segment t = I T + J is keys[off[t] .. off[t + 1])); values[n] = the
//                 scored matrix's entry.  A workgroup whose segment(s) are empty returns before it forms a tile.  The
//                 tile (with ORIENT: both tiles) is parked in LDS over the dead image, 64 rows of 68 floats each, and the
//                 threads read the listed entries from there.
//   RANK pass     u[0 .. m) = the distinct magnitudes of the positives, ascending.  Every scored entry with magnitude x
//                 is counted in counts[2 lb + (u[lb] == x)], lb = #{u < x} by a branchless binary search (the 16 searches
//                 of a lane advance together, so a step's 16 probes are in flight at once).  Integer atomics only: the
//                 counts do not depend on arrival order.  The two lowest and the two highest buckets (0, 1, 2m - 1, 2m:
//                 everything below / above all positives, and the ties with the weakest / strongest positive -- the zero
//                 columns of relu(g_j) = 0, the masked half under ORIENT) and the non-finite counter are summed per lane
//                 in registers, per workgroup in LDS, and leave with ONE global atomic each per workgroup.
// Registers and LDS of the compiled kernels: DESIGN.md section 8e.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

#include "phx_effects_tile.inc"

constexpr unsigned NSC_NAN = 0x7fc00000u;            // GATHER: a key outside the tile of its segment
constexpr size_t NSC_WS_BYTES = 64;                  // unsigned nonfinite at byte 0, padding
constexpr unsigned NSC_MAX_M = 0x7fffffffu;          // 2 m + 1 fits 32 bits

// the masked value of `a` against its partner `b`: make_mask keeps a only when |a| > |b| (false with a NaN on either side)
__device__ __forceinline__ float nsc_masked(float a, float b)
{
    const unsigned ma = __float_as_uint(a) & 0x7fffffffu, mb = __float_as_uint(b) & 0x7fffffffu;
    return (ma <= EFX_INF && mb <= EFX_INF && ma > mb) ? a : 0.f;
}

// ---------------------------------------------------------------------------------------------------------- GATHER
template <int MODE, bool ORIENT>
__global__ __launch_bounds__(EFX_THREADS) void k_gather(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                        const float *__restrict__ WaT, const float *__restrict__ g,
                                                        const float *__restrict__ y, const float *__restrict__ ph, int N, int H,
                                                        int B, const unsigned *__restrict__ keys,
                                                        const unsigned *__restrict__ off, unsigned n_keys,
                                                        float *__restrict__ values)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    int I, J;
    efx_tile_of_block(ORIENT, T, I, J);
    // the segments of tile (I, J) and, with ORIENT, of tile (J, I); offsets are clamped to the list
    unsigned fb = min(off[I * T + J], n_keys), fe = min(off[I * T + J + 1], n_keys);
    unsigned rb = 0, re = 0;
    if (ORIENT && I != J) {
        rb = min(off[J * T + I], n_keys);
        re = min(off[J * T + I + 1], n_keys);
    }
    if (fb >= fe && rb >= re) return;          // uniform over the workgroup: nothing is listed here
    const int i0 = I * EFX_TILE, j0 = J * EFX_TILE;

    f4 va[2][2], vb[2][2];
    efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
    float *ta = lds, *tb = lds;                // ta[il][jl] = M[i0 + il, j0 + jl];  tb[jl][il] = M[j0 + jl, i0 + il]
    if (ORIENT && I != J) {
        __syncthreads();                       // every wave is done with the image of tile (I, J)
        efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, j0, i0, vb);
        tb = lds + EFX_TBUF;
    }
    __syncthreads();                           // the image is dead: the parked tiles take its place
    efx_park(ta, va, tb, vb, ORIENT && I != J, iw + lc, jw + 4 * lq);
    __syncthreads();

    for (unsigned n = fb + tid; n < fe; n += EFX_THREADS) {
        const unsigned key = keys[n], i = key / (unsigned)N, j = key - i * (unsigned)N;
        const unsigned il = i - (unsigned)i0, jl = j - (unsigned)j0;
        float v = __uint_as_float(NSC_NAN);
        if (il < (unsigned)EFX_TILE && jl < (unsigned)EFX_TILE) {
            v = ta[il * EFX_TLD + jl];
            if (ORIENT) v = i == j ? 0.f : nsc_masked(v, tb[jl * EFX_TLD + il]);
        }
        values[n] = v;
    }
    for (unsigned n = rb + tid; n < re; n += EFX_THREADS) {      // ORIENT, I != J: entries (j, i) of tile (J, I)
        const unsigned key = keys[n], j = key / (unsigned)N, i = key - j * (unsigned)N;
        const unsigned il = i - (unsigned)i0, jl = j - (unsigned)j0;
        float v = __uint_as_float(NSC_NAN);
        if (il < (unsigned)EFX_TILE && jl < (unsigned)EFX_TILE) v = nsc_masked(tb[jl * EFX_TLD + il], ta[il * EFX_TLD + jl]);
        values[n] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ RANK
struct rank_args {
    const unsigned *u;             // [m] ascending, distinct
    unsigned m;
    unsigned top;                  // the largest power of two <= m
    unsigned *counts;              // [2 m + 1]
    unsigned *nonfinite;
    int diagonal;
};

// counts the up to 16 entries x[e] of this lane whose bit is set in `valid`; hot[0..3] / hot[4]: the lane's sums of the
// buckets 0, 1, 2m - 1, 2m and of the non-finite entries
__device__ __forceinline__ void nsc_rank16(const unsigned (&x)[16], unsigned valid, const rank_args &a, unsigned (&hot)[5])
{
    unsigned lb[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) lb[e] = 0;
    for (unsigned step = a.top; step; step >>= 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned probe = lb[e] + step;               // <= 2 m: no overflow (m <= NSC_MAX_M)
            if (((valid >> e) & 1u) && probe <= a.m && a.u[probe - 1] < x[e]) lb[e] = probe;
        }
    }
    const unsigned last = 2u * a.m;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (!((valid >> e) & 1u)) continue;
        if (x[e] >= EFX_INF) {
            ++hot[4];
            continue;
        }
        const unsigned b = 2u * lb[e] + ((lb[e] < a.m && a.u[lb[e]] == x[e]) ? 1u : 0u);
        if (b < 2u)
            ++hot[b];
        else if (b + 1u >= last)
            ++hot[2u + (b + 1u - last)];
        else
            atomicAdd(&a.counts[b], 1u);
    }
}

template <int MODE, bool ORIENT>
__global__ __launch_bounds__(EFX_THREADS) void k_rank(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                      const float *__restrict__ WaT, const float *__restrict__ g,
                                                      const float *__restrict__ y, const float *__restrict__ ph, int N, int H,
                                                      int B, rank_args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ unsigned wg_hot[5];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    int I, J;
    efx_tile_of_block(ORIENT, T, I, J);
    const int i0 = I * EFX_TILE, j0 = J * EFX_TILE;

    f4 va[2][2];                   // tile (I, J)
    f4 vp[2][2];                   // ORIENT: vp[ti][tj][r] = M[j, i] for the entry (i, j) of va[ti][tj][r]
    const auto zero_hot = [&] {
        if (tid < 5) wg_hot[tid] = 0;
    };
    if (ORIENT) {
        efx_tile_pair<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, I, J, iw + lc, jw + 4 * lq, va, vp, zero_hot);
    } else {
        efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
        zero_hot();
        __syncthreads();
    }

    // the scores of this lane's entries: bit 4 (2 ti + tj) + r of `fwd` for (i, j), of `rev` for (j, i)
    unsigned xf[16], xr[16];
    unsigned fwd = 0, rev = 0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int i = i0 + iw + 16 * ti + lc;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + jw + 16 * tj + 4 * lq + r;
                const int e = 4 * (2 * ti + tj) + r;
                const bool inside = i < N && j < N;
                const unsigned ma = __float_as_uint(va[ti][tj][r]) & 0x7fffffffu;
                if (inside && (i != j || a.diagonal)) fwd |= 1u << e;
                if (ORIENT) {
                    const unsigned mb = __float_as_uint(vp[ti][tj][r]) & 0x7fffffffu;
                    const bool cmp = ma <= EFX_INF && mb <= EFX_INF;
                    xf[e] = (cmp && ma > mb && i != j) ? ma : 0u;
                    xr[e] = (cmp && mb > ma) ? mb : 0u;
                    if (inside && I != J) rev |= 1u << e;
                } else {
                    xf[e] = ma;
                    xr[e] = 0u;
                }
            }
        }
    }

    unsigned hot[5] = {0u, 0u, 0u, 0u, 0u};
    nsc_rank16(xf, fwd, a, hot);
    if (ORIENT && I != J) nsc_rank16(xr, rev, a, hot);       // uniform over the workgroup
#pragma unroll
    for (int h = 0; h < 5; ++h)
        if (hot[h]) atomicAdd(&wg_hot[h], hot[h]);
    __syncthreads();
    if (tid < 5) {
        const unsigned c = wg_hot[tid];
        if (c) {
            const size_t last = 2 * (size_t)a.m;
            unsigned *dst = tid == 4 ? a.nonfinite : a.counts + (tid < 2 ? (size_t)tid : last - 1 + (tid - 2));
            atomicAdd(dst, c);
        }
    }
}

size_t netscore_lds_bytes(int H, int mode, int tiles)
{
    const size_t tile = effects_lds_bytes(H, mode), tail = (size_t)tiles * EFX_TBUF * sizeof(float);
    return tile > tail ? tile : tail;
}

template <int MODE, bool ORIENT>
int gather_launch(const phx_params *p, const float *y, const float *ph, int B, const unsigned *keys, const unsigned *off,
                  unsigned n_keys, float *values, hipStream_t st)
{
    const size_t lds = netscore_lds_bytes(p->H, MODE, ORIENT ? 2 : 1);
    if (!phxh::set_lds(k_gather<MODE, ORIENT>, lds)) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL((k_gather<MODE, ORIENT>), dim3(efx_pair_grid(p->N, ORIENT)), dim3(EFX_THREADS), lds, st, p->Ws, p->Wp,
                       p->WaT, p->g, y, ph, p->N, p->H, B, keys, off, n_keys, values);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

template <int MODE, bool ORIENT>
int rank_launch(const phx_params *p, const float *y, const float *ph, int B, const rank_args &a, hipStream_t st)
{
    const size_t lds = netscore_lds_bytes(p->H, MODE, ORIENT ? 1 : 0);
    if (!phxh::set_lds(k_rank<MODE, ORIENT>, lds)) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL((k_rank<MODE, ORIENT>), dim3(efx_pair_grid(p->N, ORIENT)), dim3(EFX_THREADS), lds, st, p->Ws, p->Wp,
                       p->WaT, p->g, y, ph, p->N, p->H, B, a);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t phx_effects_rank_workspace_bytes(int N, int H, int B, int mode)
{
    // i N + j must fit the 32 bits of a key, N^2 the 32 bits of a count
    if (!efx_pair_shape_ok(N, H) || !efx_mode_ok(mode)) return 0;
    if (mode != PHX_EFFECTS && B < 1) return 0;
    return NSC_WS_BYTES;
}

int phx_effects_gather(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, const unsigned *keys,
                       const unsigned *tile_offsets, unsigned n_keys, float *values, void *stream)
{
    if (!efx_args_ok(p, mode, y, ph, B, flags, PHX_EDGES_ORIENT | PHX_EDGES_DIAGONAL)) return PHX_ERR_BAD_ARG;
    if (!efx_pair_shape_ok(p->N, p->H)) return PHX_ERR_BAD_ARG;
    if (!keys || !tile_offsets || !values || n_keys < 1) return PHX_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    return efx_dispatch(mode, (flags & PHX_EDGES_ORIENT) != 0, y, ph, B,
                        [&](auto MODE, auto ORIENT, const float *ys, const float *phs, int Bs) {
                            return gather_launch<decltype(MODE)::value, decltype(ORIENT)::value>(p, ys, phs, Bs, keys,
                                                                                                 tile_offsets, n_keys, values, st);
                        });
}

int phx_effects_rank_counts(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, const unsigned *u,
                            unsigned m, unsigned *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!efx_args_ok(p, mode, y, ph, B, flags, PHX_EDGES_ORIENT | PHX_EDGES_DIAGONAL)) return PHX_ERR_BAD_ARG;
    if (!efx_pair_shape_ok(p->N, p->H)) return PHX_ERR_BAD_ARG;
    if (!u || !counts || m < 1 || m > NSC_MAX_M) return PHX_ERR_BAD_ARG;
    const size_t need = phx_effects_rank_workspace_bytes(p->N, p->H, B, mode);
    if (!workspace || workspace_bytes < need) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    rank_args a;
    a.u = u;
    a.m = m;
    a.top = 1u;
    while (a.top <= m / 2) a.top <<= 1;
    a.counts = counts;
    a.nonfinite = static_cast<unsigned *>(workspace);
    a.diagonal = (flags & PHX_EDGES_DIAGONAL) != 0;
    if (hipMemsetAsync(counts, 0, (2 * (size_t)m + 1) * sizeof(unsigned), st) != hipSuccess) return PHX_ERR_LAUNCH;
    if (hipMemsetAsync(a.nonfinite, 0, sizeof(unsigned), st) != hipSuccess) return PHX_ERR_LAUNCH;
    return efx_dispatch(mode, (flags & PHX_EDGES_ORIENT) != 0, y, ph, B,
                        [&](auto MODE, auto ORIENT, const float *ys, const float *phs, int Bs) {
                            return rank_launch<decltype(MODE)::value, decltype(ORIENT)::value>(p, ys, phs, Bs, a, st);
                        });
}

}  // extern "C"
