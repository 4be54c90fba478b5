// phx_neighbors.hip -- every gene's k strongest regulators (the lines are the columns of the matrix) or targets (the lines are
// its rows), with the line's degree and weighted degree, selected in the epilogue of the 64 x 64 MFMA tile engine
// (phx_effects_tile.inc) that phx_effects_matrix stores: the matrix is never stored, and every reported value is the
// efx_tile<MODE> value of its entry.  An entry M[i,j] is eligible when it is finite and non-zero, off the diagonal (unless
// PHX_EDGES_DIAGONAL), with PHX_EDGES_ORIENT strictly stronger than M[j,i] (the rules of phx_edges.hip, on the magnitude
// bits m = bits & 0x7fffffff), its regulator and its target pass their candidate masks, and m >= bits(tau).
//
//   grid          Workgroup (L, s) owns the 64 lines of line tile L and streams the tiles [s T / S, (s + 1) T / S) of the
//                 other dimension, ascending (T = ceil(N / 64), S segments).  For every streamed tile it forms tile (I, J) --
//                 (streamed, L) when the lines are targets, (L, streamed) when they are regulators -- and, with ORIENT and
//                 I != J, the partner tile (J, I); both are parked over the dead image, 64 rows of 65 floats (row-major by
//                 regulator, so a line is read along a row or along a column without bank conflicts either way).
//   selection     Four adjacent lanes share a line; each reads 16 entries of it with their partners, decides eligibility,
//                 counts, sums the magnitudes in entry order and marks the entries whose key beats the line's threshold.
//                 key = m << 32 | (0xffff - other gene) << 1 | sign: keys of one line are distinct, and comparing them
//                 orders by magnitude descending, then by the other gene ascending; the value's bits are rebuilt from it.
//                 The first lane of the four owns the line: it takes the four counts, sums and marks by shuffles (sums in
//                 lane order) and inserts the marked entries into the line's list, k unsorted keys in the workspace that
//                 only this lane touches: appended until the list is full, then over the smallest key, after which the
//                 list is read once for its new smallest key, the threshold.  Nothing of a line lives in LDS between tiles,
//                 so the selection costs the same 64 bytes of LDS in every mode and for every H and k.
//   merge         k_neighbors_merge, one wave per line: lane e holds entry e of every segment's list, k rounds of a wave
//                 maximum emit the line sorted; counts are integer sums, strengths float sums, both in segment order.
//   skipping      A workgroup whose 64 lines hold no candidate writes zero counts and forms no tile; a streamed tile
//                 without a candidate on its side is skipped before it is formed.
// No atomics at all: lists are sets selected by a total order, and every sum has an order fixed by (N, S).
// Registers and LDS of the compiled kernels: DESIGN.md section 8f.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

#include "phx_effects_tile.inc"

typedef unsigned long long u64;

constexpr int NBR_LD = 65;                           // floats of a row of a parked tile
constexpr int NBR_TBUF = EFX_TILE * NBR_LD;          // 4160 floats
constexpr int NBR_HEAD = 16;                         // floats in front of the image: the 64 candidate bytes of the streamed tile
constexpr int NBR_MAX_K = 64;
constexpr int NBR_MAX_SEG = 8;
constexpr int NBR_WORKGROUPS = 1024;                 // the segment rule aims at this many workgroups
constexpr int NBR_MERGE_LINES = EFX_THREADS / 64;    // lines of a workgroup of the merge kernel

struct nbr_args {
    const unsigned char *line_ok, *other_ok;   // [N] or null: the candidate masks of the lines' and of the streamed side
    u64 *keys;                     // [S][Np][k]
    unsigned *cnt;                 // [S][Np]
    float *str;                    // [S][Np]
    unsigned lo;                   // m >= lo
    int k, S, axis, diagonal;
};

__device__ __forceinline__ u64 nbr_key(float v, unsigned other)
{
    const unsigned bits = __float_as_uint(v);
    return ((u64)(bits & 0x7fffffffu) << 32) | (u64)(((0xffffu - other) << 1) | (bits >> 31));
}

__device__ __forceinline__ u64 nbr_shfl(u64 x, int src)
{
    const unsigned lo = __shfl((unsigned)x, src), hi = __shfl((unsigned)(x >> 32), src);
    return ((u64)hi << 32) | lo;
}

// the smallest of the k keys of a full list and where it is; four loads are in flight at a time
__device__ __forceinline__ void nbr_smallest(const u64 *list, int k, u64 &thr, int &pos)
{
    u64 best = ~0ull;
    int bp = 0;
    for (int p = 0; p < k; p += 4) {
        u64 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = p + u < k ? list[p + u] : ~0ull;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (x[u] < best) {
                best = x[u];
                bp = p + u;
            }
    }
    thr = best;
    pos = bp;
}

template <int MODE, bool ORIENT>
__global__ __launch_bounds__(EFX_THREADS) void k_neighbors(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                           const float *__restrict__ WaT, const float *__restrict__ g,
                                                           const float *__restrict__ y, const float *__restrict__ ph, int N,
                                                           int H, int B, nbr_args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char *oks = reinterpret_cast<unsigned char *>(lds);   // candidate bytes of the streamed tile
    float *img = lds + NBR_HEAD, *ta = img;
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;
    const int T = (N + EFX_TILE - 1) / EFX_TILE, Np = T * EFX_TILE;
    const int L = blockIdx.x / a.S, seg = blockIdx.x - L * a.S;
    const int t_begin = (int)((long long)seg * T / a.S), t_end = (int)((long long)(seg + 1) * T / a.S);
    const int l = tid >> 2, q = tid & 3, gl = L * EFX_TILE + l;    // this thread's line and its quarter of the entries
    const bool owner = q == 0, target_lines = a.axis == PHX_NEIGHBORS_OF_TARGET;
    const int first = lane & ~3;                                   // the owner's lane
    const size_t slot = (size_t)seg * Np + gl;
    u64 *list = a.keys + slot * a.k;

    const bool line_ok = gl < N && (!a.line_ok || a.line_ok[gl]);
    if (!__syncthreads_or(line_ok)) {          // uniform over the workgroup: no candidate among its lines
        if (owner) {
            a.cnt[slot] = 0;
            a.str[slot] = 0.f;
        }
        return;
    }
    // where entry o of this thread's line and its partner lie in the parked tiles ta[il][jl], tb[jl][il]
    const int e_base = target_lines ? l : l * NBR_LD, e_step = target_lines ? NBR_LD : 1;
    const int p_base = target_lines ? l * NBR_LD : l, p_step = target_lines ? 1 : NBR_LD;

    unsigned cnt = 0;                          // owner: the line's eligible entries, their magnitudes' sum, the list's state
    float str = 0.f;
    int fill = 0, pos = 0;
    u64 thr = 0;                               // the smallest key of a full list; 0 while there is room

    for (int t = t_begin; t < t_end; ++t) {
        const int o0 = t * EFX_TILE;
        bool any = false;
        if (tid < EFX_TILE) {
            any = o0 + tid < N && (!a.other_ok || a.other_ok[o0 + tid]);
            oks[tid] = any;
        }
        if (!__syncthreads_or(any)) continue;  // uniform: no candidate on the streamed side (nobody reads oks of this tile)
        const int i0 = target_lines ? o0 : L * EFX_TILE, j0 = target_lines ? L * EFX_TILE : o0;
        const bool two = ORIENT && i0 != j0;   // a diagonal tile is its own partner
        f4 va[2][2], vb[2][2];
        efx_tile<MODE>(img, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
        if (two) {
            __syncthreads();                   // every wave is done with the image of tile (I, J)
            efx_tile<MODE>(img, Ws, Wp, WaT, g, y, ph, N, H, B, j0, i0, vb);
        }
        __syncthreads();                       // the image is dead: the parked tiles take its place
        const float *tb = two ? ta + NBR_TBUF : ta;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int at = (iw + 16 * ti + lc) * NBR_LD + jw + 16 * tj + 4 * lq + r;
                    ta[at] = va[ti][tj][r];
                    if (two) ta[NBR_TBUF + at] = vb[ti][tj][r];
                }
        __syncthreads();

        const u64 line_thr = nbr_shfl(thr, first);
        unsigned marks = 0, c = 0;
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = 16 * q + e, go = o0 + o;
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
                ++c;
                sum += __uint_as_float(m);
                if (nbr_key(v, (unsigned)go) > line_thr) marks |= 1u << e;
            }
        }
        // the owner takes the four quarters: counts, sums in lane order, marks
        const unsigned c1 = __shfl(c, first + 1), c2 = __shfl(c, first + 2), c3 = __shfl(c, first + 3);
        const float s1 = __shfl(sum, first + 1), s2 = __shfl(sum, first + 2), s3 = __shfl(sum, first + 3);
        const unsigned m1 = __shfl(marks, first + 1), m2 = __shfl(marks, first + 2), m3 = __shfl(marks, first + 3);
        if (owner) {
            cnt += c + c1 + c2 + c3;
            str += ((sum + s1) + s2) + s3;
            u64 todo = (u64)marks | ((u64)m1 << 16) | ((u64)m2 << 32) | ((u64)m3 << 48);
            while (todo) {
                const int o = __builtin_ctzll(todo);
                todo &= todo - 1;
                const u64 key = nbr_key(ta[e_base + o * e_step], (unsigned)(o0 + o));
                if (key <= thr) continue;      // the threshold has risen since the entry was marked
                if (fill < a.k) {
                    list[fill++] = key;
                    if (fill == a.k) nbr_smallest(list, a.k, thr, pos);
                } else {
                    list[pos] = key;
                    nbr_smallest(list, a.k, thr, pos);
                }
            }
        }
        __syncthreads();                       // the parked tiles and oks are read: the next image may be staged
    }
    if (owner) {
        a.cnt[slot] = cnt;
        a.str[slot] = str;
    }
}

// one wave per line: the segments' lists (entry e of each in lane e) merged into the k strongest, sorted
__global__ __launch_bounds__(EFX_THREADS) void k_neighbors_merge(const u64 *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                                 const float *__restrict__ str, int N, int Np, int k, int S,
                                                                 int *__restrict__ gene, float *__restrict__ value,
                                                                 unsigned *__restrict__ count, float *__restrict__ strength)
{
    const int lane = threadIdx.x & 63;
    const int line = blockIdx.x * NBR_MERGE_LINES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (line >= N) return;                     // uniform over the wave
    u64 mine[NBR_MAX_SEG];
    unsigned total = 0;
    float st = 0.f;
#pragma unroll
    for (int s = 0; s < NBR_MAX_SEG; ++s) {
        mine[s] = 0;
        if (s < S) {
            const size_t slot = (size_t)s * Np + line;
            const unsigned c = cnt[slot];
            if ((unsigned)lane < min(c, (unsigned)k)) mine[s] = keys[slot * k + lane];
            total += c;
            st += str[slot];
        }
    }
    u64 res = 0;
    for (int r = 0; r < k; ++r) {
        u64 best = mine[0];
#pragma unroll
        for (int s = 1; s < NBR_MAX_SEG; ++s) best = mine[s] > best ? mine[s] : best;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)best, d), hi = __shfl_xor((unsigned)(best >> 32), d);
            const u64 other = ((u64)hi << 32) | lo;
            best = other > best ? other : best;
        }
        if (best == 0) break;                  // uniform: the lists are used up
#pragma unroll
        for (int s = 0; s < NBR_MAX_SEG; ++s)
            if (mine[s] == best) mine[s] = 0;  // keys of a line are distinct: one slot of one lane
        if (lane == r) res = best;
    }
    if (lane < k) {
        const size_t at = (size_t)line * k + lane;
        gene[at] = res ? (int)(0xffffu - ((unsigned)(res >> 1) & 0xffffu)) : -1;
        value[at] = res ? __uint_as_float((unsigned)(res >> 32) | ((unsigned)(res & 1) << 31)) : 0.f;
    }
    if (lane == 0) {
        count[line] = total;
        strength[line] = st;
    }
}

// segments of the streamed dimension: enough for NBR_WORKGROUPS workgroups, at most NBR_MAX_SEG and one per streamed tile.
// A function of N alone (PHX_NEIGHBORS_SEGMENTS=<n> forces n, clamped the same way), so the strengths are too.
int nbr_segments(int N)
{
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    int S = (NBR_WORKGROUPS + T - 1) / T;
    const char *e = getenv("PHX_NEIGHBORS_SEGMENTS");
    if (e && atoi(e) > 0) S = atoi(e);
    S = S < NBR_MAX_SEG ? S : NBR_MAX_SEG;
    return S < T ? S : T;
}

struct nbr_layout {
    size_t keys, cnt, str, total;
};

nbr_layout nbr_workspace(int N, int k, int S)
{
    const size_t Np = (size_t)((N + EFX_TILE - 1) / EFX_TILE) * EFX_TILE;
    phxh::Take take;
    nbr_layout w;
    w.keys = take((size_t)S * Np * k * sizeof(u64));
    w.cnt = take((size_t)S * Np * sizeof(unsigned));
    w.str = take((size_t)S * Np * sizeof(float));
    w.total = take.off;
    return w;
}

size_t nbr_lds_bytes(int H, int mode, bool orient)
{
    const size_t tile = effects_lds_bytes(H, mode), parked = (size_t)(orient ? 2 : 1) * NBR_TBUF * sizeof(float);
    return NBR_HEAD * sizeof(float) + (tile > parked ? tile : parked);
}

template <int MODE, bool ORIENT>
int nbr_launch(const phx_params *p, const float *y, const float *ph, int B, const nbr_args &a, hipStream_t st)
{
    const size_t lds = nbr_lds_bytes(p->H, MODE, ORIENT);
    if (!phxh::set_lds(k_neighbors<MODE, ORIENT>, lds)) return PHX_ERR_LAUNCH;
    const int T = (p->N + EFX_TILE - 1) / EFX_TILE;
    hipLaunchKernelGGL((k_neighbors<MODE, ORIENT>), dim3(T * a.S), dim3(EFX_THREADS), lds, st, p->Ws, p->Wp, p->WaT, p->g, y, ph,
                       p->N, p->H, B, a);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t phx_effects_neighbors_workspace_bytes(int N, int H, int B, int mode, int axis, int k)
{
    if (!efx_pair_shape_ok(N, H) || !efx_mode_ok(mode)) return 0;     // the other gene's index must fit 16 bits of the key
    if (mode != PHX_EFFECTS && B < 1) return 0;
    if (axis != PHX_NEIGHBORS_OF_REGULATOR && axis != PHX_NEIGHBORS_OF_TARGET) return 0;
    if (k < 1 || k > NBR_MAX_K) return 0;
    return nbr_workspace(N, k, nbr_segments(N)).total;
}

int phx_effects_neighbors(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int axis, int k,
                          float tau, const unsigned char *regulator_ok, const unsigned char *target_ok, int *gene, float *value,
                          unsigned *count, float *strength, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!efx_args_ok(p, mode, y, ph, B, flags, PHX_EDGES_ORIENT | PHX_EDGES_DIAGONAL)) return PHX_ERR_BAD_ARG;
    if (!efx_pair_shape_ok(p->N, p->H)) return PHX_ERR_BAD_ARG;
    if (axis != PHX_NEIGHBORS_OF_REGULATOR && axis != PHX_NEIGHBORS_OF_TARGET) return PHX_ERR_BAD_ARG;
    if (k < 1 || k > NBR_MAX_K) return PHX_ERR_BAD_ARG;
    unsigned lo = 0;
    std::memcpy(&lo, &tau, sizeof lo);
    if (!(tau >= 0.f) || lo >= EFX_INF) return PHX_ERR_BAD_ARG;         // +0 (no threshold) or positive and finite
    if (!gene || !value || !count || !strength) return PHX_ERR_BAD_ARG;
    const int S = nbr_segments(p->N);
    const nbr_layout w = nbr_workspace(p->N, k, S);
    if (!workspace || workspace_bytes < w.total) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    const bool target_lines = axis == PHX_NEIGHBORS_OF_TARGET;
    nbr_args a;
    a.line_ok = target_lines ? target_ok : regulator_ok;
    a.other_ok = target_lines ? regulator_ok : target_ok;
    a.keys = reinterpret_cast<u64 *>(ws + w.keys);
    a.cnt = reinterpret_cast<unsigned *>(ws + w.cnt);
    a.str = reinterpret_cast<float *>(ws + w.str);
    a.lo = lo;
    a.k = k;
    a.S = S;
    a.axis = axis;
    a.diagonal = (flags & PHX_EDGES_DIAGONAL) != 0;
    const int rc = efx_dispatch(mode, (flags & PHX_EDGES_ORIENT) != 0, y, ph, B,
                                [&](auto MODE, auto ORIENT, const float *ys, const float *phs, int Bs) {
                                    return nbr_launch<decltype(MODE)::value, decltype(ORIENT)::value>(p, ys, phs, Bs, a, st);
                                });
    if (rc != PHX_OK) return rc;
    const int N = p->N, Np = (N + EFX_TILE - 1) / EFX_TILE * EFX_TILE;
    hipLaunchKernelGGL(k_neighbors_merge, dim3((N + NBR_MERGE_LINES - 1) / NBR_MERGE_LINES), dim3(EFX_THREADS), 0, st, a.keys,
                       a.cnt, a.str, N, Np, k, S, gene, value, count, strength);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // extern "C"
