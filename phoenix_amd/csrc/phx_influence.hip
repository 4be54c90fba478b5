// phx_influence.hip -- scoring pass of the gene-influence scan (find_gene_influences.py:64-77) over the solver's own
// output block  sol [T, 2 * pairs * B, N]:  call 2j of B rows is the unperturbed solve of pair j, call 2j + 1 the
// perturbed one.  For every pair j and target gene n
//     s[j, n]   = sum over outputs tau = 1 .. T-1 and rows b < B of | sol[tau, 2jB + b, n] - sol[tau, (2j+1)B + b, n] |
//     scores[j] = ( sum over n != genes[j] of s[j, n] ) / ((T-1) B (N-1))                       (:74-75)
// in one read of the block, on the front end of phx_screen_score.inc: two streams (the calls of a pair), one term, one
// held column.  W takes enough waves to keep the loads of every CU in flight when pairs * N is small.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/phoenix_hip.h"

namespace {

#include "phx_screen_score.inc"

constexpr int INFL_MAX_WAVES = 16;      // waves of a workgroup (1024 threads)
constexpr int INFL_WAVE_TARGET = 2048;  // waves a launch should have before rows stop being split: 8 per CU on 256 CUs
constexpr int INFL_UNROLL = 4;          // row pairs in flight per wave: 8 loads of 1 KiB

// the unperturbed row of a pair and, `call` floats on, the perturbed one: one address serves both
struct InflTerm {
    static constexpr int NS = 2, NQ = 1;
    const float *q;      // row 0 of output time 0 of the unperturbed call
    size_t slab, call;   // floats of one output time of the block / of one call in it
    __device__ __forceinline__ void seek(int cl) { q += slab + cl; }
    template <bool QUADS>
    __device__ __forceinline__ void load(f4 (&v)[NS], int tau, size_t ro, int nc) const
    {
        const float *p = q + (size_t)tau * slab + ro;
        v[0] = QUADS ? load4(p) : load_n(p, nc);
        v[1] = QUADS ? load4(p + call) : load_n(p + call, nc);
    }
    static __device__ __forceinline__ void add(f4 (&acc)[NQ], const f4 (&v)[NS]) { acc[0] += abs4(v[0] - v[1]); }
};

// s [pairs, N] (not normalised)
__global__ __launch_bounds__(INFL_MAX_WAVES * 64) void k_influence_sum(const float *__restrict__ sol, float *__restrict__ s,
                                                                      int T, int B, int N)
{
    const int j = blockIdx.y;
    const size_t call = (size_t)B * N;
    float *const out[1] = {s};
    scr_walk<InflTerm, INFL_UNROLL, INFL_MAX_WAVES>({sol + (size_t)j * 2 * call, (size_t)gridDim.y * 2 * call, call}, out, j,
                                                    T, B, N);
}

// scores[pair0 + blockIdx.x] from row pair0 + blockIdx.x of s; scale != 0: the row becomes targets = s / M in place
__global__ __launch_bounds__(SCR_SCORE_THREADS) void k_influence_score(float *s, float *__restrict__ scores, ScrIdx<1> genes,
                                                                      int pair0, int N, int M, int scale)
{
    float *const mat[1] = {s};
    float *const sc[1] = {scores};
    scr_score<1, 1, 1>(mat, sc, genes, pair0, N, M, scale);
}

bool influence_shape_ok(int T, int pairs, int B, int N)
{
    return scr_shape_ok(T, pairs, B, N, 2) && 2LL * pairs * B <= INT_MAX;
}

}  // namespace

extern "C" {

size_t phx_influence_workspace_bytes(int T, int pairs, int B, int N)
{
    return influence_shape_ok(T, pairs, B, N) ? scr_matrix_bytes(pairs, N) : 0;
}

int phx_influence_scores(const float *sol, int T, int pairs, int B, int N, const int *genes_host, float *scores,
                         float *targets, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!sol || !scores || !genes_host || !influence_shape_ok(T, pairs, B, N) || !scr_in_range(genes_host, pairs, N))
        return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_influence_workspace_bytes(T, pairs, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *s = targets ? targets : (float *)workspace;
    const int W = scr_waves_filling(T, pairs, B, N, INFL_MAX_WAVES, INFL_WAVE_TARGET);
    hipLaunchKernelGGL(k_influence_sum, scr_sum_grid(N, pairs), dim3(W * 64), 0, st, sol, s, T, B, N);
    if (!scr_launched()) return PHX_ERR_LAUNCH;
    return scr_for_chunks<1>(pairs, [&](int p0, int np) {
        const ScrIdx<1> g = scr_pack<1>(p0, np, [&](int, int j) { return genes_host[j]; });
        hipLaunchKernelGGL(k_influence_score, dim3(np), dim3(SCR_SCORE_THREADS), 0, st, s, scores, g, p0, N, (T - 1) * B,
                           targets ? 1 : 0);
        return scr_launched();
    });
}

}  // extern "C"
