// phx_knockout.hip -- scoring pass of a knockout screen: K clamped solves (phx_odeint_clamped) against ONE unperturbed
// solve.  base [T, B, N] is the baseline's output block, sol [T, K * B, N] that of K calls of B rows.  For knockout k and
// target gene n, with d = sol[tau, kB + b, n] - base[tau, b, n] over outputs tau = 1 .. T-1 and rows b < B:
//     shift[k, n]     = mean of d         (signed: the target goes up or down)
//     magnitude[k, n] = mean of |d|
//     scores[k]       = mean of magnitude[k, n] over n != genes[k]          (find_gene_influences.py:74-75)
// The shape of phx_influence.hip, one baseline instead of a pair layout: sol is read once (its tau = 0 slab not at all),
// the baseline rows a workgroup needs are those its neighbours in k read too (they stay in the L2), two plain launches:
//
//   k_knockout_sum    grid (ceil(N / 256), K), W waves per workgroup.  A lane owns four adjacent gene columns (one 16-byte
//                     load per row and lane) and adds d and |d| of its rows in row order.  The (T-1) B rows are dealt
//                     round-robin to the W waves; the W partial sums meet in LDS and wave 0 adds them in wave order.  W
//                     depends on the shape alone, so the order of every sum is fixed: no atomics, two runs agree bit for
//                     bit.
//   k_knockout_score  one workgroup per knockout: thread t adds the |d| sums of columns t, t + 256, ... in order, skipping
//                     column genes[k] by index, then a fixed LDS tree; it also scales the sums to means where the caller
//                     wants the matrices.  The score is formed from the unscaled sums either way.
//
// The ragged tail (N % 4 != 0): the lane that owns the last 1..3 columns loads the quad that ENDS at column N - 1 and
// stores only its own columns, so the hot loop has one shape for every lane and nothing is read past a row's end.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstring>

#include "../../include/phoenix_hip.h"

namespace {

constexpr int KO_TILE = 256;          // gene columns of a workgroup: one quad per lane
constexpr int KO_MAX_WAVES = 16;      // waves of a workgroup (1024 threads)
constexpr int KO_WAVE_TARGET = 2048;  // waves a launch should have before rows stop being split: 8 per CU on 256 CUs
constexpr int KO_UNROLL = 4;          // rows in flight per wave: 8 loads of 1 KiB
constexpr int KO_SCORE_THREADS = 256;
constexpr int KO_GENES_PER_LAUNCH = 256;   // clamped-gene indices travel as kernel arguments (1 KiB)

typedef float f4 __attribute__((ext_vector_type(4)));

struct KoGenes {
    int g[KO_GENES_PER_LAUNCH];
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

__device__ __forceinline__ f4 abs4(f4 d) { return f4{fabsf(d.x), fabsf(d.y), fabsf(d.z), fabsf(d.w)}; }

// row r = (tau - 1) * B + b of the wave's round-robin walk: (tau, b) -> the next one, `step` rows on
__device__ __forceinline__ void advance(int &tau, int &b, int step, int B)
{
    b += step;
    while (b >= B) {
        b -= B;
        ++tau;
    }
}

// the lane's quad `v` to out[0 .. 3], or its owned columns of it (nc < 4: the quad starts `skip` columns early)
__device__ __forceinline__ void store_owned(float *out, f4 v, int nc, int skip)
{
    if (nc == 4) {
        __builtin_memcpy(out, &v, sizeof(f4));
    } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k >= skip && k < skip + nc) out[k] = e[k];
    }
}

// sa [K, N]: sums of |d|; ss [K, N]: sums of d, or null (not wanted)
__global__ __launch_bounds__(KO_MAX_WAVES * 64) void k_knockout_sum(const float *__restrict__ base, const float *__restrict__ sol,
                                                                    float *__restrict__ sa, float *__restrict__ ss, int T, int B,
                                                                    int N)
{
    __shared__ f4 part[2][KO_MAX_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int k = blockIdx.y;
    const int c0 = blockIdx.x * KO_TILE + lane * 4;       // first column this lane owns
    const int nc = min(4, N - c0);                        // columns it owns (<= 0: none)
    const bool quads = N >= 4;
    const int cl = (quads && nc > 0 && nc < 4) ? N - 4 : c0;   // first column it loads
    const size_t bslab = (size_t)B * N;                   // floats of one output time of the baseline
    const size_t sslab = (size_t)gridDim.y * bslab;       // ... of the K calls
    const float *bq = base + bslab + cl;                  // tau = 1, row 0
    const float *sq = sol + sslab + (size_t)k * bslab + cl;
    const int M = (T - 1) * B;
    f4 accA = {0.f, 0.f, 0.f, 0.f}, accS = accA;
    if (nc > 0) {
        int tau = 0, b = 0, r = wv;
        advance(tau, b, wv, B);
        if (quads) {
            for (; r + (KO_UNROLL - 1) * nwv < M; r += KO_UNROLL * nwv) {
                f4 u[KO_UNROLL], p[KO_UNROLL];
#pragma unroll
                for (int i = 0; i < KO_UNROLL; ++i) {
                    u[i] = load4(bq + (size_t)tau * bslab + (size_t)b * N);
                    p[i] = load4(sq + (size_t)tau * sslab + (size_t)b * N);
                    advance(tau, b, nwv, B);
                }
#pragma unroll
                for (int i = 0; i < KO_UNROLL; ++i) {
                    const f4 d = p[i] - u[i];
                    accS += d;
                    accA += abs4(d);
                }
            }
            for (; r < M; r += nwv) {
                const f4 d = load4(sq + (size_t)tau * sslab + (size_t)b * N) - load4(bq + (size_t)tau * bslab + (size_t)b * N);
                accS += d;
                accA += abs4(d);
                advance(tau, b, nwv, B);
            }
        } else {
            for (; r < M; r += nwv) {
                const f4 d = load_n(sq + (size_t)tau * sslab + (size_t)b * N, nc) -
                             load_n(bq + (size_t)tau * bslab + (size_t)b * N, nc);
                accS += d;
                accA += abs4(d);
                advance(tau, b, nwv, B);
            }
        }
    }
    part[0][wv][lane] = accA;
    part[1][wv][lane] = accS;
    __syncthreads();
    if (wv != 0 || nc <= 0) return;
    f4 totA = part[0][0][lane], totS = part[1][0][lane];
    for (int w = 1; w < nwv; ++w) {
        totA += part[0][w][lane];
        totS += part[1][w][lane];
    }
    // the loaded quad starts c0 - cl columns before the first owned one (0 when N < 4)
    store_owned(sa + (size_t)k * N + cl, totA, nc, c0 - cl);
    if (ss) store_owned(ss + (size_t)k * N + cl, totS, nc, c0 - cl);
}

// scores[k0 + blockIdx.x] from row k0 + blockIdx.x of sa; scale_a / scale_s: the rows of sa / ss become means in place
__global__ __launch_bounds__(KO_SCORE_THREADS) void k_knockout_score(float *sa, float *ss, float *__restrict__ scores,
                                                                    KoGenes genes, int k0, int N, int M, int scale_a,
                                                                    int scale_s)
{
    __shared__ float red[KO_SCORE_THREADS];
    const int tid = threadIdx.x;
    const int gene = genes.g[blockIdx.x];
    float *rowa = sa + (size_t)(k0 + blockIdx.x) * N;
    float *rows = scale_s ? ss + (size_t)(k0 + blockIdx.x) * N : nullptr;
    const double dM = (double)M;
    float acc = 0.f;
    for (int n = tid; n < N; n += KO_SCORE_THREADS) {
        const float v = rowa[n];
        if (n != gene) acc += v;
        if (scale_a) rowa[n] = (float)((double)v / dM);
        if (scale_s) rows[n] = (float)((double)rows[n] / dM);
    }
    red[tid] = acc;
    for (int h = KO_SCORE_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];
    }
    if (tid == 0) scores[k0 + blockIdx.x] = (float)((double)red[0] / (dM * (double)(N - 1)));
}

bool knockout_shape_ok(int T, int K, int B, int N)
{
    return T >= 2 && K >= 1 && B >= 1 && N >= 2 && K <= 65535 && (long long)(T - 1) * B <= INT_MAX &&
           (long long)K * B <= INT_MAX;
}

// waves per workgroup: rows are split over more waves until the launch has KO_WAVE_TARGET of them (a function of the
// shape alone: the summation order must not depend on the device)
int knockout_waves(int T, int K, int B, int N)
{
    const long long wgs = (long long)((N + KO_TILE - 1) / KO_TILE) * K, M = (long long)(T - 1) * B;
    int W = 1;
    while (W < KO_MAX_WAVES && wgs * W < KO_WAVE_TARGET && 2 * W <= M) W *= 2;
    return W;
}

}  // namespace

extern "C" {

size_t phx_knockout_effects_workspace_bytes(int T, int K, int B, int N)
{
    if (!knockout_shape_ok(T, K, B, N)) return 0;
    return ((size_t)K * N * sizeof(float) + 255) / 256 * 256;
}

int phx_knockout_effects(const float *base, const float *sol, int T, int K, int B, int N, const int *genes_host,
                         float *scores, float *shift, float *magnitude, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    if (!base || !sol || !scores || !genes_host || !knockout_shape_ok(T, K, B, N)) return PHX_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k)
        if (genes_host[k] < 0 || genes_host[k] >= N) return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_knockout_effects_workspace_bytes(T, K, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *sa = magnitude ? magnitude : (float *)workspace;   // the |d| sums: the score needs them either way
    const int W = knockout_waves(T, K, B, N);
    hipLaunchKernelGGL(k_knockout_sum, dim3((N + KO_TILE - 1) / KO_TILE, K), dim3(W * 64), 0, st, base, sol, sa, shift, T, B, N);
    if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    for (int k0 = 0; k0 < K; k0 += KO_GENES_PER_LAUNCH) {
        const int nk = K - k0 < KO_GENES_PER_LAUNCH ? K - k0 : KO_GENES_PER_LAUNCH;
        KoGenes g;
        memset(&g, 0, sizeof(g));
        memcpy(g.g, genes_host + k0, sizeof(int) * (size_t)nk);
        hipLaunchKernelGGL(k_knockout_score, dim3(nk), dim3(KO_SCORE_THREADS), 0, st, sa, shift, scores, g, k0, N, (T - 1) * B,
                           magnitude ? 1 : 0, shift ? 1 : 0);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}

}  // extern "C"
