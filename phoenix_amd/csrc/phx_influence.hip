// phx_influence.hip -- scoring pass of the gene-influence scan (find_gene_influences.py:64-77) over the solver's own
// output block  sol [T, 2 * pairs * B, N]:  call 2j of B rows is the unperturbed solve of pair j, call 2j + 1 the
// perturbed one.  For every pair j and target gene n
//     s[j, n]   = sum over outputs tau = 1 .. T-1 and rows b < B of | sol[tau, 2jB + b, n] - sol[tau, (2j+1)B + b, n] |
//     scores[j] = ( sum over n != genes[j] of s[j, n] ) / ((T-1) B (N-1))                       (:74-75)
// in one read of the block (the tau = 0 slab, the initial states, is never touched) and two plain launches:
//
//   k_influence_sum    grid (ceil(N / 256), pairs), W waves per workgroup.  A lane owns four adjacent gene columns (one
//                      16-byte load per row and lane, 1 KiB per wave instruction; gfx950 global loads need dword
//                      alignment only, so rows of an N that is no multiple of 4 are read the same way) and adds its terms
//                      in row order.  The (T-1) B row pairs are dealt round-robin to the W waves; the W partial sums meet
//                      in LDS and wave 0 adds them in wave order.  W depends on the shape alone (enough waves to keep the
//                      loads of every CU in flight when pairs * N is small), so the order of every sum is fixed: no
//                      atomics, two runs agree bit for bit.
//   k_influence_score  one workgroup per pair: thread t adds columns t, t + 256, ... in order, skipping column genes[j] by
//                      index, then a fixed LDS tree; it also scales s to the per-target means when the caller wants them.
//
// The ragged tail (N % 4 != 0): the lane that owns the last 1..3 columns loads the quad that ENDS at column N - 1 and
// stores only its own columns, so the hot loop has one shape for every lane and nothing is read past a row's end.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstring>

#include "../../include/phoenix_hip.h"

namespace {

constexpr int INFL_TILE = 256;          // gene columns of a workgroup: one quad per lane
constexpr int INFL_MAX_WAVES = 16;      // waves of a workgroup (1024 threads)
constexpr int INFL_WAVE_TARGET = 2048;  // waves a launch should have before rows stop being split: 8 per CU on 256 CUs
constexpr int INFL_UNROLL = 4;          // row pairs in flight per wave: 8 loads of 1 KiB
constexpr int INFL_SCORE_THREADS = 256;
constexpr int INFL_GENES_PER_LAUNCH = 256;   // perturbed-gene indices travel as kernel arguments (1 KiB)

typedef float f4 __attribute__((ext_vector_type(4)));

struct InflGenes {
    int g[INFL_GENES_PER_LAUNCH];
};

// four floats from a dword-aligned address
__device__ __forceinline__ f4 load4(const float *p)
{
    f4 v;
    __builtin_memcpy(&v, p, sizeof(f4));
    return v;
}

// the columns a lane holds when N < 4 (one lane, no quad fits a row): element loads
__device__ __forceinline__ f4 load_n(const float *p, int n)
{
    f4 v = {0.f, 0.f, 0.f, 0.f};
    v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    return v;
}

__device__ __forceinline__ f4 absdiff(f4 a, f4 b)
{
    const f4 d = a - b;
    return f4{fabsf(d.x), fabsf(d.y), fabsf(d.z), fabsf(d.w)};
}

// row pair r = (tau - 1) * B + b of the wave's round-robin walk: (tau, b) -> the next one, `step` pairs on
__device__ __forceinline__ void advance(int &tau, int &b, int step, int B)
{
    b += step;
    while (b >= B) {
        b -= B;
        ++tau;
    }
}

// s [pairs, N] (not normalised).  slab = 2 * pairs * B * N, the floats of one output time.
__global__ __launch_bounds__(INFL_MAX_WAVES * 64) void k_influence_sum(const float *__restrict__ sol, float *__restrict__ s,
                                                                      int T, int B, int N)
{
    __shared__ f4 part[INFL_MAX_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int j = blockIdx.y;
    const int c0 = blockIdx.x * INFL_TILE + lane * 4;     // first column this lane owns
    const int nc = min(4, N - c0);                        // columns it owns (<= 0: none)
    const bool quads = N >= 4;
    const int cl = (quads && nc > 0 && nc < 4) ? N - 4 : c0;   // first column it loads
    const size_t rowpair = (size_t)B * N;                 // unperturbed row -> perturbed row
    const size_t slab = (size_t)gridDim.y * 2 * rowpair;
    const float *base = sol + slab + (size_t)j * 2 * rowpair + cl;   // tau = 1, row 0 of the unperturbed call
    const int M = (T - 1) * B;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    if (nc > 0) {
        int tau = 0, b = 0, r = wv;
        advance(tau, b, wv, B);
        if (quads) {
            for (; r + (INFL_UNROLL - 1) * nwv < M; r += INFL_UNROLL * nwv) {
                f4 u[INFL_UNROLL], p[INFL_UNROLL];
#pragma unroll
                for (int k = 0; k < INFL_UNROLL; ++k) {
                    const float *q = base + (size_t)tau * slab + (size_t)b * N;
                    u[k] = load4(q);
                    p[k] = load4(q + rowpair);
                    advance(tau, b, nwv, B);
                }
#pragma unroll
                for (int k = 0; k < INFL_UNROLL; ++k) acc += absdiff(u[k], p[k]);
            }
            for (; r < M; r += nwv) {
                const float *q = base + (size_t)tau * slab + (size_t)b * N;
                acc += absdiff(load4(q), load4(q + rowpair));
                advance(tau, b, nwv, B);
            }
        } else {
            for (; r < M; r += nwv) {
                const float *q = base + (size_t)tau * slab + (size_t)b * N;
                acc += absdiff(load_n(q, nc), load_n(q + rowpair, nc));
                advance(tau, b, nwv, B);
            }
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv != 0 || nc <= 0) return;
    f4 tot = part[0][lane];
    for (int w = 1; w < nwv; ++w) tot += part[w][lane];
    float *out = s + (size_t)j * N + cl;
    if (nc == 4) {
        __builtin_memcpy(out, &tot, sizeof(f4));
    } else {
        // the loaded quad starts c0 - cl columns before the first owned one (0 when N < 4)
        const float e[4] = {tot.x, tot.y, tot.z, tot.w};
        const int skip = c0 - cl;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k >= skip && k < skip + nc) out[k] = e[k];
    }
}

// scores[pair0 + blockIdx.x] from row pair0 + blockIdx.x of s; scale != 0: the row becomes targets = s / M in place
__global__ __launch_bounds__(INFL_SCORE_THREADS) void k_influence_score(float *s, float *__restrict__ scores, InflGenes genes,
                                                                       int pair0, int N, int M, int scale)
{
    __shared__ float red[INFL_SCORE_THREADS];
    const int tid = threadIdx.x;
    const int gene = genes.g[blockIdx.x];
    float *row = s + (size_t)(pair0 + blockIdx.x) * N;
    const double dM = (double)M;
    float acc = 0.f;
    for (int n = tid; n < N; n += INFL_SCORE_THREADS) {
        const float v = row[n];
        if (n != gene) acc += v;
        if (scale) row[n] = (float)((double)v / dM);
    }
    red[tid] = acc;
    for (int h = INFL_SCORE_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];
    }
    if (tid == 0) scores[pair0 + blockIdx.x] = (float)((double)red[0] / (dM * (double)(N - 1)));
}

bool influence_shape_ok(int T, int pairs, int B, int N)
{
    return T >= 2 && pairs >= 1 && B >= 1 && N >= 2 && pairs <= 65535 && (long long)(T - 1) * B <= INT_MAX &&
           2LL * pairs * B <= INT_MAX;
}

// waves per workgroup: rows are split over more waves until the launch has INFL_WAVE_TARGET of them (a function of
// the shape alone: the summation order must not depend on the device)
int influence_waves(int T, int pairs, int B, int N)
{
    const long long wgs = (long long)((N + INFL_TILE - 1) / INFL_TILE) * pairs, M = (long long)(T - 1) * B;
    int W = 1;
    while (W < INFL_MAX_WAVES && wgs * W < INFL_WAVE_TARGET && 2 * W <= M) W *= 2;
    return W;
}

}  // namespace

extern "C" {

size_t phx_influence_workspace_bytes(int T, int pairs, int B, int N)
{
    if (!influence_shape_ok(T, pairs, B, N)) return 0;
    return ((size_t)pairs * N * sizeof(float) + 255) / 256 * 256;
}

int phx_influence_scores(const float *sol, int T, int pairs, int B, int N, const int *genes_host, float *scores,
                         float *targets, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!sol || !scores || !genes_host || !influence_shape_ok(T, pairs, B, N)) return PHX_ERR_BAD_ARG;
    for (int j = 0; j < pairs; ++j)
        if (genes_host[j] < 0 || genes_host[j] >= N) return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_influence_workspace_bytes(T, pairs, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *s = targets ? targets : (float *)workspace;
    const int W = influence_waves(T, pairs, B, N);
    hipLaunchKernelGGL(k_influence_sum, dim3((N + INFL_TILE - 1) / INFL_TILE, pairs), dim3(W * 64), 0, st, sol, s, T, B, N);
    if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    for (int p0 = 0; p0 < pairs; p0 += INFL_GENES_PER_LAUNCH) {
        const int np = pairs - p0 < INFL_GENES_PER_LAUNCH ? pairs - p0 : INFL_GENES_PER_LAUNCH;
        InflGenes g;
        memset(&g, 0, sizeof(g));
        memcpy(g.g, genes_host + p0, sizeof(int) * (size_t)np);
        hipLaunchKernelGGL(k_influence_score, dim3(np), dim3(INFL_SCORE_THREADS), 0, st, s, scores, g, p0, N, (T - 1) * B,
                           targets ? 1 : 0);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}

}  // extern "C"
