// phx_epistasis.hip -- scoring pass of a PAIR knockout screen: K calls that hold two genes each (phx_odeint_clamped_sets)
// against the unperturbed solve AND the two single-gene calls of every pair.  base [T, B, N] is the baseline's output
// block, singles [T, G * B, N] that of G single-gene calls, sol [T, K * B, N] that of the K pair calls; pair k holds the
// genes of singles ia[k] and ib[k].  With d_x = x - base (float32) over outputs tau = 1 .. T-1 and rows b < B, and
//     e = d_ab - (d_a + d_b)                  (the sum first: symmetric in a and b, swapping the pair changes no bit)
// the outputs are
//     shift[k, n]                 = mean of d_ab          magnitude[k, n]             = mean of |d_ab|
//     interaction[k, n]           = mean of e             interaction_magnitude[k, n] = mean of |e|
//     scores[k] / interaction_scores[k] = mean of magnitude / interaction_magnitude [k, n] over n not in {a, b}
// On the front end of phx_screen_score.inc: four streams (the baseline, the two singles, pair call k), four terms, two
// held columns (N >= 3).  What is this pass's own:
//   W depends on (T, B, N) alone -- not on K, unlike phx_knockout.hip's -- so a pair's sums do not depend on which other
//   pairs share its call: the same pairs split over several calls agree bit for bit.  The baseline and single rows a
//   workgroup needs are those its neighbours in k read too (they stay in the L2).
//   The two held columns are skipped BY INDEX because on column a, e is -d_b[a]: no interaction, and it dominates the
//   row -- subtracting it from a total afterwards loses the float32 score.
//   The pairs go chunk by chunk, a sum and a score launch each: the indices of both travel as kernel arguments.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/phoenix_hip.h"

namespace {

#include "phx_screen_score.inc"

constexpr int EP_MAX_WAVES = 8;       // waves of a workgroup (512 threads; their partial sums take 32 KiB of LDS)
constexpr int EP_UNROLL = 2;          // rows in flight per wave: 8 loads of 1 KiB

// v: the rows of the baseline, single a, single b and the pair; acc: sums of |d_ab|, |e|, d_ab, e
struct EpTerm : ScrStreams<4> {
    static constexpr int NQ = 4;
    static __device__ __forceinline__ void add(f4 (&acc)[NQ], const f4 (&v)[NS])
    {
        const f4 dab = v[3] - v[0], da = v[1] - v[0], db = v[2] - v[0];
        const f4 e = dab - (da + db);
        acc[2] += dab;
        acc[0] += abs4(dab);
        acc[3] += e;
        acc[1] += abs4(e);
    }
};

// am / ei [K, N]: sums of |d_ab| / |e| (always); sh / in [K, N]: sums of d_ab / e, or null (not wanted).  Pair
// blockIdx.y of the launch is pair k0 + blockIdx.y of the call (pr: its two singles); Ks / Gs: the calls of sol / singles
// (their row strides).
__global__ __launch_bounds__(EP_MAX_WAVES * 64) void k_epistasis_sum(const float *__restrict__ base,
                                                                     const float *__restrict__ singles,
                                                                     const float *__restrict__ sol, float *__restrict__ am,
                                                                     float *__restrict__ ei, float *__restrict__ sh,
                                                                     float *__restrict__ in, ScrIdx<2> pr, int k0, int Ks,
                                                                     int Gs, int T, int B, int N)
{
    const int k = k0 + blockIdx.y;
    const size_t bslab = (size_t)B * N;                   // floats of one output time of the baseline
    const EpTerm term = {{{base, singles + (size_t)pr.g[0][blockIdx.y] * bslab, singles + (size_t)pr.g[1][blockIdx.y] * bslab,
                           sol + (size_t)k * bslab},
                          {bslab, (size_t)Gs * bslab, (size_t)Gs * bslab, (size_t)Ks * bslab}}};
    float *const out[4] = {am, ei, sh, in};
    scr_walk<EpTerm, EP_UNROLL, EP_MAX_WAVES>(term, out, k, T, B, N);
}

// scores[k] / iscores[k], k = k0 + blockIdx.x, from row k of am / ei; a row of a matrix whose scale flag is set becomes
// means in place (scale bits: 1 am, 2 ei, 4 sh, 8 in)
__global__ __launch_bounds__(SCR_SCORE_THREADS) void k_epistasis_score(float *am, float *ei, float *sh, float *in,
                                                                      float *__restrict__ scores, float *__restrict__ iscores,
                                                                      ScrIdx<2> held, int k0, int N, int M, int scale)
{
    float *const mat[4] = {am, ei, sh, in};
    float *const sc[2] = {scores, iscores};
    scr_score<2, 2, 4>(mat, sc, held, k0, N, M, scale);
}

bool epistasis_shape_ok(int T, int K, int G, int B, int N)
{
    return scr_shape_ok(T, K, B, N, 3) && G >= 2 && (long long)G * B <= INT_MAX;
}

// waves per workgroup: a function of (T, B, N) alone -- neither the device nor the number of pairs in the call may
// change the order of a sum.  A wave should have at least four rows; wide rows have many workgroups already.
int epistasis_waves(int T, int B, int N)
{
    const long long M = (long long)(T - 1) * B;
    const int cap = N > 4 * SCR_TILE ? 4 : EP_MAX_WAVES;
    int W = 1;
    while (W < cap && 8 * W <= M) W *= 2;
    return W;
}

}  // namespace

extern "C" {

size_t phx_knockout_epistasis_workspace_bytes(int T, int K, int G, int B, int N)
{
    return epistasis_shape_ok(T, K, G, B, N) ? 2 * scr_matrix_bytes(K, N) : 0;
}

int phx_knockout_epistasis(const float *base, const float *singles, const float *sol, int T, int K, int G, int B, int N,
                           const int *ia_host, const int *ib_host, const int *genes_host, float *scores,
                           float *interaction_scores, float *shift, float *magnitude, float *interaction,
                           float *interaction_magnitude, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!base || !singles || !sol || !ia_host || !ib_host || !genes_host || !scores || !interaction_scores ||
        !epistasis_shape_ok(T, K, G, B, N) || !scr_in_range(genes_host, G, N) || !scr_in_range(ia_host, K, G) ||
        !scr_in_range(ib_host, K, G))
        return PHX_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k)
        if (ia_host[k] == ib_host[k]) return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_knockout_epistasis_workspace_bytes(T, K, G, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // the |d_ab| and |e| sums: the scores need them either way
    float *am = magnitude ? magnitude : (float *)workspace;
    float *ei = interaction_magnitude ? interaction_magnitude : (float *)((char *)workspace + scr_matrix_bytes(K, N));
    const int W = epistasis_waves(T, B, N);
    const int scale = (magnitude ? 1 : 0) | (interaction_magnitude ? 2 : 0) | (shift ? 4 : 0) | (interaction ? 8 : 0);
    return scr_for_chunks<2>(K, [&](int k0, int nk) {
        const ScrIdx<2> idx = scr_pack<2>(k0, nk, [&](int l, int k) { return (l ? ib_host : ia_host)[k]; });
        const ScrIdx<2> held = scr_pack<2>(k0, nk, [&](int l, int k) { return genes_host[(l ? ib_host : ia_host)[k]]; });
        hipLaunchKernelGGL(k_epistasis_sum, scr_sum_grid(N, nk), dim3(W * 64), 0, st, base, singles, sol, am, ei, shift,
                           interaction, idx, k0, K, G, T, B, N);
        if (!scr_launched()) return false;
        hipLaunchKernelGGL(k_epistasis_score, dim3(nk), dim3(SCR_SCORE_THREADS), 0, st, am, ei, shift, interaction, scores,
                           interaction_scores, held, k0, N, (T - 1) * B, scale);
        return scr_launched();
    });
}

}  // extern "C"
