// phx_apply.hip -- products of a block of R <= 32 vectors with the regulator -> target matrix, taken after the element-wise
// rules of phx_neighbors.hip and without the matrix: out[n, r] = sum over the eligible entries of line n of
// w(entry) * V[other gene, r], the lines being the columns of the matrix (PHX_NEIGHBORS_OF_TARGET: M^T V, scores flow
// regulator -> target) or its rows (PHX_NEIGHBORS_OF_REGULATOR: M V), w the entry, its magnitude or 1.  It is k_neighbors with
// a sum in place of the selection: the same line-tile x segment grid, the same parked tiles (64 rows of 65 floats over the
// dead image, the partner tile alongside under ORIENT), the same eligibility on the magnitude bits m = bits & 0x7fffffff and
// the same skipping of line tiles and streamed tiles without a candidate; k_neighbors itself is not touched, the parking
// and the eligibility are restated here.
//
//   products      Lane l of every wave owns line l of the workgroup's 64; wave q takes entries 16 q .. 16 q + 15 of every
//                 streamed tile.  The streamed tile's 64 x R slice of V lies in LDS, rows of 32 floats in front of the
//                 image, so all lanes of a wave read one address (a broadcast) while they read the parked tile along a row
//                 or a column, 65 floats apart: neither read has a bank conflict.  An eligible entry adds
//                 fmaf(w, V[other, r], acc[r]) to the lane's R accumulators; an ineligible one is skipped, not multiplied
//                 by zero, so a non-finite entry of M never reaches a sum and a non-finite V[g, r] reaches only the lines
//                 with an eligible entry at g.
//   sum order     acc[r] of (line, q) runs over the streamed tiles of the segment ascending and over the wave's 16 entries
//                 of each ascending; after the last tile the four waves' accumulators meet in LDS and wave 0 stores
//                 ((a0 + a1) + a2) + a3 as the segment's partial; k_apply_sum adds the S partials in segment order.  The
//                 order of column r is fixed by (N, S) alone: it depends neither on R nor on where in the block r stands.
// No atomics; plain global stores.  Registers and LDS of the compiled kernels: DESIGN.md section 8m.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

#include "phx_effects_tile.inc"

constexpr int APL_LD = 65;                           // floats of a row of a parked tile
constexpr int APL_TBUF = EFX_TILE * APL_LD;          // 4160 floats
constexpr int APL_MAX_R = 32;                        // columns of V per call
constexpr int APL_OKS = 16;                          // floats in front of the slice: the 64 candidate bytes of the streamed tile
constexpr int APL_HEAD = APL_OKS + EFX_TILE * APL_MAX_R;   // ... and the slice of V, [64][32]: the image follows
constexpr int APL_RND = 8;                           // columns of a round of the final exchange between the waves
constexpr int APL_XLD = APL_RND + 1;                 // floats of a lane's row in the exchange buffer
constexpr int APL_MAX_SEG = 8;
constexpr int APL_WORKGROUPS = 1024;                 // the segment rule of phx_neighbors.hip
static_assert(3 * EFX_TILE * APL_XLD <= APL_TBUF, "the exchange buffer lies over the parked tile");
static_assert(APL_HEAD % 4 == 0, "the image stays 16-byte aligned");

struct apl_args {
    const unsigned char *line_ok, *other_ok;   // [N] or null: the candidate masks of the lines' and of the streamed side
    const float *V;                // [N][R]
    float *part;                   // [S][Np][R]
    unsigned lo;                   // m >= lo
    int R, S, axis, diagonal, weight;
};

template <int MODE, bool ORIENT>
__global__ __launch_bounds__(EFX_THREADS) void k_apply(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                       const float *__restrict__ WaT, const float *__restrict__ g,
                                                       const float *__restrict__ y, const float *__restrict__ ph, int N, int H,
                                                       int B, apl_args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char *oks = reinterpret_cast<unsigned char *>(lds);   // candidate bytes of the streamed tile
    float *vs = lds + APL_OKS;                                      // its slice of V, vs[o * 32 + r]
    float *img = lds + APL_HEAD, *ta = img;
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;
    const int T = (N + EFX_TILE - 1) / EFX_TILE, Np = T * EFX_TILE;
    const int L = blockIdx.x / a.S, seg = blockIdx.x - L * a.S;
    const int t_begin = (int)((long long)seg * T / a.S), t_end = (int)((long long)(seg + 1) * T / a.S);
    const int l = lane, gl = L * EFX_TILE + l;                     // this lane's line; wave wv takes entries 16 wv ..
    const bool target_lines = a.axis == PHX_NEIGHBORS_OF_TARGET;
    const int R = a.R;
    float *part = a.part + ((size_t)seg * Np + gl) * R;            // gl < Np always

    const bool line_ok = gl < N && (!a.line_ok || a.line_ok[gl]);
    if (!__syncthreads_or(line_ok)) {          // uniform over the workgroup: no candidate among its lines
        if (wv == 0)
            for (int r = 0; r < R; ++r) part[r] = 0.f;
        return;
    }
    // where entry o of this lane's line and its partner lie in the parked tiles ta[il][jl], tb[jl][il]
    const int e_base = target_lines ? l : l * APL_LD, e_step = target_lines ? APL_LD : 1;
    const int p_base = target_lines ? l * APL_LD : l, p_step = target_lines ? 1 : APL_LD;

    float acc[APL_MAX_R];
#pragma unroll
    for (int r = 0; r < APL_MAX_R; ++r) acc[r] = 0.f;

    for (int t = t_begin; t < t_end; ++t) {
        const int o0 = t * EFX_TILE;
        bool any = false;
        if (tid < EFX_TILE) {
            any = o0 + tid < N && (!a.other_ok || a.other_ok[o0 + tid]);
            oks[tid] = any;
        }
        if (!__syncthreads_or(any)) continue;  // uniform: no candidate on the streamed side (nobody reads oks of this tile)
        // rows o0 .. o0 + 63 of V, zeros beyond column R and beyond row N (those rows are never read from memory); the
        // barriers of the tile in between make the slice visible
        for (int s = tid; s < EFX_TILE * APL_MAX_R; s += EFX_THREADS) {
            const int row = s >> 5, col = s & 31;
            vs[s] = (col < R && o0 + row < N) ? a.V[(size_t)(o0 + row) * R + col] : 0.f;
        }
        const int i0 = target_lines ? o0 : L * EFX_TILE, j0 = target_lines ? L * EFX_TILE : o0;
        const bool two = ORIENT && i0 != j0;   // a diagonal tile is its own partner
        f4 va[2][2], vb[2][2];
        efx_tile<MODE>(img, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
        if (two) {
            __syncthreads();                   // every wave is done with the image of tile (I, J)
            efx_tile<MODE>(img, Ws, Wp, WaT, g, y, ph, N, H, B, j0, i0, vb);
        }
        __syncthreads();                       // the image is dead: the parked tiles take its place
        const float *tb = two ? ta + APL_TBUF : ta;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int at = (iw + 16 * ti + lc) * APL_LD + jw + 16 * tj + 4 * lq + r;
                    ta[at] = va[ti][tj][r];
                    if (two) ta[APL_TBUF + at] = vb[ti][tj][r];
                }
        __syncthreads();

#pragma unroll 2
        for (int e = 0; e < 16; ++e) {
            const int o = 16 * wv + e, go = o0 + o;
            const float v = ta[e_base + o * e_step];
            const unsigned m = __float_as_uint(v) & 0x7fffffffu;
            bool ok = line_ok && oks[o] && m != 0 && m < EFX_INF && m >= a.lo;
            if (ORIENT) {
                const unsigned mb = __float_as_uint(tb[p_base + o * p_step]) & 0x7fffffffu;
                ok = ok && go != gl && mb <= EFX_INF && m > mb;
            } else {
                ok = ok && (go != gl || a.diagonal);
            }
            if (ok) {
                const float w = a.weight == PHX_APPLY_UNIT ? 1.0f : (a.weight == PHX_APPLY_ABS ? __uint_as_float(m) : v);
                const f4 *row = reinterpret_cast<const f4 *>(vs + o * APL_MAX_R);
#pragma unroll
                for (int c = 0; c < APL_MAX_R / 4; ++c)
                    if (4 * c < R) {           // uniform
                        const f4 x = row[c];
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[4 * c + u] = fmaf(w, x[u], acc[4 * c + u]);
                    }
            }
        }
        __syncthreads();                       // the parked tiles, the slice and oks are read: the next image may be staged
    }

    // the four waves' accumulators of a line meet in LDS, APL_RND columns at a time; wave 0 adds them in wave order
    float *xb = img;
#pragma unroll
    for (int c0 = 0; c0 < APL_MAX_R; c0 += APL_RND) {
        if (c0 >= R) break;                    // uniform
        if (wv > 0) {
#pragma unroll
            for (int u = 0; u < APL_RND; ++u) xb[((wv - 1) * EFX_TILE + l) * APL_XLD + u] = acc[c0 + u];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int u = 0; u < APL_RND; ++u) {
                float s = acc[c0 + u];
#pragma unroll
                for (int q = 0; q < 3; ++q) s += xb[(q * EFX_TILE + l) * APL_XLD + u];
                if (c0 + u < R) part[c0 + u] = s;
            }
        }
        __syncthreads();                       // the round is read: the next may be written
    }
}

// out[n, r] = the S partials of (n, r), added in segment order
__global__ __launch_bounds__(EFX_THREADS) void k_apply_sum(const float *__restrict__ part, size_t stride, size_t count, int S,
                                                           float *__restrict__ out)
{
    const size_t at = (size_t)blockIdx.x * EFX_THREADS + threadIdx.x;
    if (at >= count) return;
    float s = part[at];
    for (int q = 1; q < S; ++q) s += part[q * stride + at];
    out[at] = s;
}

// the segment rule of phx_neighbors.hip (nbr_segments), with its per-call switch: a function of N alone
int apl_segments(int N)
{
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    int S = (APL_WORKGROUPS + T - 1) / T;
    const char *e = getenv("PHX_NEIGHBORS_SEGMENTS");
    if (e && atoi(e) > 0) S = atoi(e);
    S = S < APL_MAX_SEG ? S : APL_MAX_SEG;
    return S < T ? S : T;
}

size_t apl_padded(int N) { return (size_t)((N + EFX_TILE - 1) / EFX_TILE) * EFX_TILE; }

// the S partial blocks [Np][R]
size_t apl_workspace(int N, int R, int S) { return (size_t)S * apl_padded(N) * R * sizeof(float); }

size_t apl_lds_bytes(int H, int mode, bool orient)
{
    const size_t tile = effects_lds_bytes(H, mode), parked = (size_t)(orient ? 2 : 1) * APL_TBUF * sizeof(float);
    return APL_HEAD * sizeof(float) + (tile > parked ? tile : parked);
}

bool apl_shape_ok(int N, int H, int B, int mode, int axis, int R)
{
    if (!efx_pair_shape_ok(N, H) || !efx_mode_ok(mode)) return false;
    if (mode != PHX_EFFECTS && B < 1) return false;
    if (axis != PHX_NEIGHBORS_OF_REGULATOR && axis != PHX_NEIGHBORS_OF_TARGET) return false;
    return R >= 1 && R <= APL_MAX_R;
}

template <int MODE, bool ORIENT>
int apl_launch(const phx_params *p, const float *y, const float *ph, int B, const apl_args &a, hipStream_t st)
{
    const size_t lds = apl_lds_bytes(p->H, MODE, ORIENT);
    if (lds > phxh::LDS_BUDGET || !phxh::set_lds(k_apply<MODE, ORIENT>, lds)) return PHX_ERR_LAUNCH;
    const int T = (p->N + EFX_TILE - 1) / EFX_TILE;
    hipLaunchKernelGGL((k_apply<MODE, ORIENT>), dim3(T * a.S), dim3(EFX_THREADS), lds, st, p->Ws, p->Wp, p->WaT, p->g, y, ph,
                       p->N, p->H, B, a);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t phx_effects_apply_workspace_bytes(int N, int H, int B, int mode, int axis, int R)
{
    if (!apl_shape_ok(N, H, B, mode, axis, R)) return 0;
    return apl_workspace(N, R, apl_segments(N));
}

int phx_effects_apply(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int axis, int weight,
                      float tau, const unsigned char *regulator_ok, const unsigned char *target_ok, const float *V, int R,
                      float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!efx_args_ok(p, mode, y, ph, B, flags, PHX_EDGES_ORIENT | PHX_EDGES_DIAGONAL)) return PHX_ERR_BAD_ARG;
    if (!apl_shape_ok(p->N, p->H, mode == PHX_EFFECTS ? 1 : B, mode, axis, R)) return PHX_ERR_BAD_ARG;
    if (weight != PHX_APPLY_VALUE && weight != PHX_APPLY_ABS && weight != PHX_APPLY_UNIT) return PHX_ERR_BAD_ARG;
    unsigned lo = 0;
    std::memcpy(&lo, &tau, sizeof lo);
    if (!(tau >= 0.f) || lo >= EFX_INF) return PHX_ERR_BAD_ARG;         // +0 (no threshold) or positive and finite
    if (!V || !out) return PHX_ERR_BAD_ARG;
    const int N = p->N, S = apl_segments(N);
    if (!workspace || workspace_bytes < apl_workspace(N, R, S)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool target_lines = axis == PHX_NEIGHBORS_OF_TARGET;
    apl_args a;
    a.line_ok = target_lines ? target_ok : regulator_ok;
    a.other_ok = target_lines ? regulator_ok : target_ok;
    a.V = V;
    a.part = static_cast<float *>(workspace);
    a.lo = lo;
    a.R = R;
    a.S = S;
    a.axis = axis;
    a.diagonal = (flags & PHX_EDGES_DIAGONAL) != 0;
    a.weight = weight;
    const int rc = efx_dispatch(mode, (flags & PHX_EDGES_ORIENT) != 0, y, ph, B,
                                [&](auto MODE, auto ORIENT, const float *ys, const float *phs, int Bs) {
                                    return apl_launch<decltype(MODE)::value, decltype(ORIENT)::value>(p, ys, phs, Bs, a, st);
                                });
    if (rc != PHX_OK) return rc;
    const size_t count = (size_t)N * R;
    hipLaunchKernelGGL(k_apply_sum, dim3((unsigned)((count + EFX_THREADS - 1) / EFX_THREADS)), dim3(EFX_THREADS), 0, st, a.part,
                       apl_padded(N) * R, count, S, out);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // extern "C"
