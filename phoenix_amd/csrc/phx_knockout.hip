// phx_knockout.hip -- scoring pass of a knockout screen: K clamped solves (phx_odeint_clamped) against ONE unperturbed
// solve.  base [T, B, N] is the baseline's output block, sol [T, K * B, N] that of K calls of B rows.  For knockout k and
// target gene n, with d = sol[tau, kB + b, n] - base[tau, b, n] over outputs tau = 1 .. T-1 and rows b < B:
//     shift[k, n]     = mean of d         (signed: the target goes up or down)
//     magnitude[k, n] = mean of |d|
//     scores[k]       = mean of magnitude[k, n] over n != genes[k]          (find_gene_influences.py:74-75)
// On the front end of phx_screen_score.inc: two streams (the baseline and call k), two terms, one held column.  sol is
// read once; the baseline rows a workgroup needs are those its neighbours in k read too (they stay in the L2).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/phoenix_hip.h"

namespace {

#include "phx_screen_score.inc"

constexpr int KO_MAX_WAVES = 16;      // waves of a workgroup (1024 threads)
constexpr int KO_WAVE_TARGET = 2048;  // waves a launch should have before rows stop being split: 8 per CU on 256 CUs
constexpr int KO_UNROLL = 4;          // rows in flight per wave: 8 loads of 1 KiB

struct KoTerm : ScrStreams<2> {   // v: the baseline's and the knockout's row; acc: sums of |d|, of d
    static constexpr int NQ = 2;
    static __device__ __forceinline__ void add(f4 (&acc)[NQ], const f4 (&v)[NS])
    {
        const f4 d = v[1] - v[0];
        acc[1] += d;
        acc[0] += abs4(d);
    }
};

// sa [K, N]: sums of |d|; ss [K, N]: sums of d, or null (not wanted)
__global__ __launch_bounds__(KO_MAX_WAVES * 64) void k_knockout_sum(const float *__restrict__ base, const float *__restrict__ sol,
                                                                    float *__restrict__ sa, float *__restrict__ ss, int T, int B,
                                                                    int N)
{
    const int k = blockIdx.y;
    const size_t bslab = (size_t)B * N;                   // floats of one output time of the baseline
    float *const out[2] = {sa, ss};
    scr_walk<KoTerm, KO_UNROLL, KO_MAX_WAVES>({{{base, sol + (size_t)k * bslab}, {bslab, (size_t)gridDim.y * bslab}}}, out, k,
                                              T, B, N);
}

// scores[k0 + blockIdx.x] from row k0 + blockIdx.x of sa; scale bits 1 / 2: the rows of sa / ss become means in place
__global__ __launch_bounds__(SCR_SCORE_THREADS) void k_knockout_score(float *sa, float *ss, float *__restrict__ scores,
                                                                     ScrIdx<1> genes, int k0, int N, int M, int scale)
{
    float *const mat[2] = {sa, ss};
    float *const sc[1] = {scores};
    scr_score<1, 1, 2>(mat, sc, genes, k0, N, M, scale);
}

bool knockout_shape_ok(int T, int K, int B, int N) { return scr_shape_ok(T, K, B, N, 2); }

}  // namespace

extern "C" {

size_t phx_knockout_effects_workspace_bytes(int T, int K, int B, int N)
{
    return knockout_shape_ok(T, K, B, N) ? scr_matrix_bytes(K, N) : 0;
}

int phx_knockout_effects(const float *base, const float *sol, int T, int K, int B, int N, const int *genes_host,
                         float *scores, float *shift, float *magnitude, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    if (!base || !sol || !scores || !genes_host || !knockout_shape_ok(T, K, B, N) || !scr_in_range(genes_host, K, N))
        return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_knockout_effects_workspace_bytes(T, K, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *sa = magnitude ? magnitude : (float *)workspace;   // the |d| sums: the score needs them either way
    const int W = scr_waves_filling(T, K, B, N, KO_MAX_WAVES, KO_WAVE_TARGET);
    hipLaunchKernelGGL(k_knockout_sum, scr_sum_grid(N, K), dim3(W * 64), 0, st, base, sol, sa, shift, T, B, N);
    if (!scr_launched()) return PHX_ERR_LAUNCH;
    return scr_for_chunks<1>(K, [&](int k0, int nk) {
        const ScrIdx<1> g = scr_pack<1>(k0, nk, [&](int, int k) { return genes_host[k]; });
        hipLaunchKernelGGL(k_knockout_score, dim3(nk), dim3(SCR_SCORE_THREADS), 0, st, sa, shift, scores, g, k0, N, (T - 1) * B,
                           (magnitude ? 1 : 0) | (shift ? 2 : 0));
        return scr_launched();
    });
}

}  // extern "C"
