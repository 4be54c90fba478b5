// phx_edges.hip -- the strongest regulator -> target edges of the matrices of phx_effects.hip, selected in the epilogue of
// the same 64 x 64 MFMA tile engine (phx_effects_tile.inc): the matrix is never stored, every pass recomputes its tiles.
// An entry M[i,j] is eligible when it is finite and non-zero, off the diagonal (unless PHX_EDGES_DIAGONAL) and, with
// PHX_EDGES_ORIENT, strictly stronger than M[j,i] (make_mask of extract_model_matrix_PHOENIX.py:29-37: the diagonal and
// both directions of an equally strong pair are dropped; a NaN partner loses the comparison).  All tests are made on the
// magnitude bits m = bits & 0x7fffffff, which order as the magnitudes do for every non-NaN float.
//
//   tiles         Without ORIENT a workgroup owns tile (I, J) of the T x T tile grid.  With ORIENT it owns the unordered pair
//                 I <= J (T (T + 1) / 2 workgroups): it forms tile (I, J), keeps it in 16 registers, forms tile (J, I) in the
//                 same image, writes that one to LDS (64 rows of 68 floats, 17 KiB over the dead image: a lane's four
//                 partner rows lie 16 banks apart) and reads it back transposed, so that the lane that holds M[i,j] also
//                 holds M[j,i] and decides both directions of the gene pair, once.  A diagonal tile is its own partner.
//                 That sequence is efx_tile_pair of phx_effects_tile.inc, which k_rank (phx_netscore.hip) shares.
//                 Both tiles come from efx_tile<MODE>, the code that k_effects stores: every value has the bits that
//                 phx_effects_matrix writes for that entry (chain k ascending, b ascending, mean, then relu(g_j)).
//   COUNT pass    A 4096-bin histogram of m: level 0 on its top 12 bits (m >> 19), level 1 on the next 12 ((m >> 7) & 4095)
//                 of the entries of level-0 bin `prefix`.  Counted in LDS (16 KiB beside the transposed tile), then one
//                 integer global atomic per non-empty bin and workgroup: integer sums do not depend on arrival order.
//   EMIT pass     Every eligible entry with m >= bits(tau) is appended to (keys, values): a lane marks its up to 32
//                 entries, a wave scan turns the marks into offsets, and ONE atomic per wave on the global cursor reserves
//                 the wave's slots.  key = (0x7fffffff - m) << 32 | (i N + j): sorting the keys ascending orders the edges
//                 by magnitude descending, then regulator, then target, whatever order the waves arrived in.  Entries past
//                 `capacity` are counted and not written.
// Registers and LDS of the compiled kernels: DESIGN.md section 8d.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <type_traits>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

#include "phx_effects_tile.inc"

constexpr int EDG_BINS = 4096;
constexpr size_t EDG_WS_BYTES = (EDG_BINS + 16) * sizeof(unsigned);   // the histogram, the cursor, padding

struct edges_args {
    unsigned *hist;                // [EDG_BINS]
    unsigned *cursor;
    unsigned long long *keys;      // [capacity]
    float *values;                 // [capacity]
    unsigned capacity;
    unsigned lo;                   // EMIT: m >= lo
    unsigned prefix;               // COUNT, level 1: (m >> 19) == prefix
    int pass, level, diagonal;
};

template <int MODE, bool ORIENT>
__global__ __launch_bounds__(EFX_THREADS) void k_edges(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                       const float *__restrict__ WaT, const float *__restrict__ g,
                                                       const float *__restrict__ y, const float *__restrict__ ph, int N, int H,
                                                       int B, edges_args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    int I, J;
    efx_tile_of_block(ORIENT, T, I, J);
    const int i0 = I * EFX_TILE, j0 = J * EFX_TILE;

    f4 va[2][2];                   // tile (I, J)
    f4 vp[2][2];                   // ORIENT: vp[ti][tj][r] = M[j, i] for the entry (i, j) of va[ti][tj][r]
    unsigned *hist = reinterpret_cast<unsigned *>(lds + (ORIENT ? EFX_TBUF : 0));     // behind the transposed tile
    const auto zero_hist = [=] {
        if (a.pass == PHX_EDGES_COUNT)
            for (int b = tid; b < EDG_BINS; b += EFX_THREADS) hist[b] = 0;
    };
    if (ORIENT) {
        efx_tile_pair<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, I, J, iw + lc, jw + 4 * lq, va, vp, zero_hist);
    } else {
        efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
        __syncthreads();           // the image is dead: the histogram takes its place
        zero_hist();
        __syncthreads();
    }

    // which of this lane's entries take part in this pass: bit 4 (2 ti + tj) + r of `fwd` for (i, j), of `rev` for (j, i)
    const bool count = a.pass == PHX_EDGES_COUNT;
    unsigned fwd = 0, rev = 0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int i = i0 + iw + 16 * ti + lc;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + jw + 16 * tj + 4 * lq + r;
                const unsigned bit = 1u << (4 * (2 * ti + tj) + r);
                const bool inside = i < N && j < N;
                const unsigned ma = __float_as_uint(va[ti][tj][r]) & 0x7fffffffu;
                bool ef, er = false;
                unsigned mb = 0;
                if (ORIENT) {
                    mb = __float_as_uint(vp[ti][tj][r]) & 0x7fffffffu;
                    ef = inside && i != j && ma != 0 && ma < EFX_INF && mb <= EFX_INF && ma > mb;
                    er = inside && I != J && mb != 0 && mb < EFX_INF && ma <= EFX_INF && mb > ma;
                } else {
                    ef = inside && ma != 0 && ma < EFX_INF && (i != j || a.diagonal);
                }
                if (count) {
                    if (a.level) {
                        ef = ef && (ma >> 19) == a.prefix;
                        er = er && (mb >> 19) == a.prefix;
                    }
                } else {
                    ef = ef && ma >= a.lo;
                    er = er && mb >= a.lo;
                }
                if (ef) fwd |= bit;
                if (er) rev |= bit;
            }
        }
    }

    if (count) {
        const int shift = a.level ? 7 : 19;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned bit = 1u << (4 * t + r);
                if (fwd & bit) atomicAdd(&hist[((__float_as_uint(va[t >> 1][t & 1][r]) & 0x7fffffffu) >> shift) & (EDG_BINS - 1)], 1u);
                if (ORIENT && (rev & bit))
                    atomicAdd(&hist[((__float_as_uint(vp[t >> 1][t & 1][r]) & 0x7fffffffu) >> shift) & (EDG_BINS - 1)], 1u);
            }
        __syncthreads();
        for (int b = tid; b < EDG_BINS; b += EFX_THREADS) {
            const unsigned c = hist[b];
            if (c) atomicAdd(&a.hist[b], c);
        }
        return;
    }

    // EMIT: offsets inside the wave by an inclusive scan of the lanes' counts, one atomic for the wave's total
    const unsigned mine = __popc(fwd) + __popc(rev);
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const unsigned total = __shfl(incl, 63);
    if (total == 0) return;
    unsigned base = 0;
    if (lane == 63) base = atomicAdd(a.cursor, total);
    unsigned pos = __shfl(base, 63) + incl - mine;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const unsigned i = i0 + iw + 16 * ti + lc;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned j = j0 + jw + 16 * tj + 4 * lq + r;
                const unsigned bit = 1u << (4 * (2 * ti + tj) + r);
                if (fwd & bit) {
                    if (pos < a.capacity) {
                        const float v = va[ti][tj][r];
                        const unsigned m = __float_as_uint(v) & 0x7fffffffu;
                        a.keys[pos] = ((unsigned long long)(0x7fffffffu - m) << 32) | (i * (unsigned)N + j);
                        a.values[pos] = v;
                    }
                    ++pos;
                }
                if (ORIENT && (rev & bit)) {
                    if (pos < a.capacity) {
                        const float v = vp[ti][tj][r];
                        const unsigned m = __float_as_uint(v) & 0x7fffffffu;
                        a.keys[pos] = ((unsigned long long)(0x7fffffffu - m) << 32) | (j * (unsigned)N + i);
                        a.values[pos] = v;
                    }
                    ++pos;
                }
            }
        }
    }
}

size_t edges_lds_bytes(int H, int mode, bool orient, int pass)
{
    const size_t tile = effects_lds_bytes(H, mode);
    const size_t tail = ((orient ? EFX_TBUF : 0) + (pass == PHX_EDGES_COUNT ? EDG_BINS : 0)) * sizeof(float);
    return tile > tail ? tile : tail;
}

template <int MODE, bool ORIENT>
int edges_launch(const phx_params *p, const float *y, const float *ph, int B, const edges_args &a, hipStream_t st)
{
    const size_t lds = edges_lds_bytes(p->H, MODE, ORIENT, a.pass);
    if (!phxh::set_lds(k_edges<MODE, ORIENT>, lds)) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL((k_edges<MODE, ORIENT>), dim3(efx_pair_grid(p->N, ORIENT)), dim3(EFX_THREADS), lds, st, p->Ws, p->Wp,
                       p->WaT, p->g, y, ph, p->N, p->H, B, a);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t phx_effects_edges_workspace_bytes(int N, int H, int B, int mode)
{
    if (!efx_pair_shape_ok(N, H) || !efx_mode_ok(mode)) return 0;     // i N + j must fit 32 bits of the key
    if (mode != PHX_EFFECTS && B < 1) return 0;
    return EDG_WS_BYTES;
}

int phx_effects_edges(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int pass, int level,
                      unsigned prefix, float tau, long long *keys, float *values, unsigned capacity, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    if (!efx_args_ok(p, mode, y, ph, B, flags, PHX_EDGES_ORIENT | PHX_EDGES_DIAGONAL)) return PHX_ERR_BAD_ARG;
    if (!efx_pair_shape_ok(p->N, p->H)) return PHX_ERR_BAD_ARG;
    unsigned lo = 0;
    if (pass == PHX_EDGES_COUNT) {
        // level-0 bins from 0xff0 up hold infinities and NaNs, which are never eligible
        if (level != 0 && level != 1) return PHX_ERR_BAD_ARG;
        if (level == 1 && prefix >= (EFX_INF >> 19)) return PHX_ERR_BAD_ARG;
    } else if (pass == PHX_EDGES_EMIT) {
        if (!keys || !values || capacity < 1) return PHX_ERR_BAD_ARG;
        std::memcpy(&lo, &tau, sizeof lo);
        if (!(tau > 0.f) || lo >= EFX_INF) return PHX_ERR_BAD_ARG;      // tau positive and finite (subnormals count)
    } else {
        return PHX_ERR_BAD_ARG;
    }
    const size_t need = phx_effects_edges_workspace_bytes(p->N, p->H, B, mode);
    if (!workspace || workspace_bytes < need) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    edges_args a;
    a.hist = static_cast<unsigned *>(workspace);
    a.cursor = a.hist + EDG_BINS;
    a.keys = reinterpret_cast<unsigned long long *>(keys);
    a.values = values;
    a.capacity = capacity;
    a.lo = lo;
    a.prefix = prefix;
    a.pass = pass;
    a.level = level;
    a.diagonal = (flags & PHX_EDGES_DIAGONAL) != 0;
    const hipError_t e = pass == PHX_EDGES_COUNT ? hipMemsetAsync(a.hist, 0, EDG_BINS * sizeof(unsigned), st)
                                                 : hipMemsetAsync(a.cursor, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return PHX_ERR_LAUNCH;
    return efx_dispatch(mode, (flags & PHX_EDGES_ORIENT) != 0, y, ph, B,
                        [&](auto MODE, auto ORIENT, const float *ys, const float *phs, int Bs) {
                            return edges_launch<decltype(MODE)::value, decltype(ORIENT)::value>(p, ys, phs, Bs, a, st);
                        });
}

}  // extern "C"
