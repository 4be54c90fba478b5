// phx_epistasis.hip -- scoring pass of a PAIR knockout screen: K calls that hold two genes each (phx_odeint_clamped_sets)
// against the unperturbed solve AND the two single-gene calls of every pair.  base [T, B, N] is the baseline's output
// block, singles [T, G * B, N] that of G single-gene calls, sol [T, K * B, N] that of the K pair calls; pair k holds the
// genes of singles ia[k] and ib[k].  With d_x = x - base (float32) over outputs tau = 1 .. T-1 and rows b < B, and
//     e = d_ab - (d_a + d_b)                  (the sum first: symmetric in a and b, swapping the pair changes no bit)
// the outputs are
//     shift[k, n]                 = mean of d_ab          magnitude[k, n]             = mean of |d_ab|
//     interaction[k, n]           = mean of e             interaction_magnitude[k, n] = mean of |e|
//     scores[k] / interaction_scores[k] = mean of magnitude / interaction_magnitude [k, n] over n not in {a, b}
// The shape of phx_knockout.hip, with three more streams per row:
//
//   k_epistasis_sum    grid (ceil(N / 256), K), W waves per workgroup.  A lane owns four adjacent gene columns (16-byte
//                      loads) and adds d_ab, |d_ab|, e and |e| of its rows in row order.  The (T-1) B rows are dealt
//                      round-robin to the W waves; the partial sums meet in LDS and wave 0 adds them in wave order.  W
//                      depends on (T, B, N) alone -- not on K, unlike phx_knockout.hip's -- so a pair's sums do not
//                      depend on which other pairs share its call: no atomics, two runs agree bit for bit, and so do
//                      the same pairs split over several calls.  The baseline and single rows a workgroup needs are
//                      those its neighbours in k read too (they stay in the L2).
//   k_epistasis_score  one workgroup per pair: thread t adds the |d_ab| and |e| sums of columns t, t + 256, ... in
//                      order, skipping the two held columns BY INDEX (on column a, e is -d_b[a]: no interaction, and it
//                      dominates the row -- subtracting it from a total afterwards loses the float32 score), then a
//                      fixed LDS tree; it also scales the sums to means where the caller wants the matrices.  The scores
//                      are formed from the unscaled sums either way.
//
// The ragged tail (N % 4 != 0): the lane that owns the last 1..3 columns loads the quad that ENDS at column N - 1 and
// stores only its own columns (N >= 3 is required, N == 3 takes element loads).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstring>

#include "../../include/phoenix_hip.h"

namespace {

constexpr int EP_TILE = 256;          // gene columns of a workgroup: one quad per lane
constexpr int EP_MAX_WAVES = 8;       // waves of a workgroup (512 threads; their partial sums take 32 KiB of LDS)
constexpr int EP_UNROLL = 2;          // rows in flight per wave: 8 loads of 1 KiB
constexpr int EP_SCORE_THREADS = 256;
constexpr int EP_PAIRS_PER_LAUNCH = 128;   // single indices / held genes travel as kernel arguments (1 KiB)

typedef float f4 __attribute__((ext_vector_type(4)));

struct EpPairs {
    int a[EP_PAIRS_PER_LAUNCH], b[EP_PAIRS_PER_LAUNCH];
};

// four floats from a dword-aligned address
__device__ __forceinline__ f4 load4(const float *p)
{
    f4 v;
    __builtin_memcpy(&v, p, sizeof(f4));
    return v;
}

// the three columns of a row when N == 3 (one lane, no quad fits a row): element loads
__device__ __forceinline__ f4 load_3(const float *p) { return f4{p[0], p[1], p[2], 0.f}; }

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

struct EpAcc {
    f4 sd, ad, se, ae;   // sums of d_ab, |d_ab|, e, |e|
    __device__ __forceinline__ void add(f4 u, f4 pa, f4 pb, f4 pab)
    {
        const f4 dab = pab - u, da = pa - u, db = pb - u;
        const f4 e = dab - (da + db);
        sd += dab;
        ad += abs4(dab);
        se += e;
        ae += abs4(e);
    }
};

// am / ei [K, N]: sums of |d_ab| / |e| (always); sh / in [K, N]: sums of d_ab / e, or null (not wanted).  Pair
// blockIdx.y of the launch is pair k0 + blockIdx.y of the call; Ks / Gs: the calls of sol / singles (their row strides).
__global__ __launch_bounds__(EP_MAX_WAVES * 64) void k_epistasis_sum(const float *__restrict__ base,
                                                                     const float *__restrict__ singles,
                                                                     const float *__restrict__ sol, float *__restrict__ am,
                                                                     float *__restrict__ ei, float *__restrict__ sh,
                                                                     float *__restrict__ in, EpPairs pr, int k0, int Ks,
                                                                     int Gs, int T, int B, int N)
{
    __shared__ f4 part[4][EP_MAX_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int k = k0 + blockIdx.y;
    const int c0 = blockIdx.x * EP_TILE + lane * 4;       // first column this lane owns
    const int nc = min(4, N - c0);                        // columns it owns (<= 0: none)
    const bool quads = N >= 4;
    const int cl = (quads && nc > 0 && nc < 4) ? N - 4 : c0;   // first column it loads
    const size_t bslab = (size_t)B * N;                   // floats of one output time of the baseline
    const size_t sslab = (size_t)Ks * bslab;              // ... of the K pair calls
    const size_t gslab = (size_t)Gs * bslab;              // ... of the G single calls
    const float *bq = base + bslab + cl;                  // tau = 1, row 0
    const float *sq = sol + sslab + (size_t)k * bslab + cl;
    const float *aq = singles + gslab + (size_t)pr.a[blockIdx.y] * bslab + cl;
    const float *cq = singles + gslab + (size_t)pr.b[blockIdx.y] * bslab + cl;
    const int M = (T - 1) * B;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    EpAcc acc{zero, zero, zero, zero};
    if (nc > 0) {
        int tau = 0, b = 0, r = wv;
        advance(tau, b, wv, B);
        if (quads) {
            for (; r + (EP_UNROLL - 1) * nwv < M; r += EP_UNROLL * nwv) {
                f4 u[EP_UNROLL], pa[EP_UNROLL], pb[EP_UNROLL], pab[EP_UNROLL];
#pragma unroll
                for (int i = 0; i < EP_UNROLL; ++i) {
                    const size_t ro = (size_t)b * N;
                    u[i] = load4(bq + (size_t)tau * bslab + ro);
                    pa[i] = load4(aq + (size_t)tau * gslab + ro);
                    pb[i] = load4(cq + (size_t)tau * gslab + ro);
                    pab[i] = load4(sq + (size_t)tau * sslab + ro);
                    advance(tau, b, nwv, B);
                }
#pragma unroll
                for (int i = 0; i < EP_UNROLL; ++i) acc.add(u[i], pa[i], pb[i], pab[i]);
            }
            for (; r < M; r += nwv) {
                const size_t ro = (size_t)b * N;
                acc.add(load4(bq + (size_t)tau * bslab + ro), load4(aq + (size_t)tau * gslab + ro),
                        load4(cq + (size_t)tau * gslab + ro), load4(sq + (size_t)tau * sslab + ro));
                advance(tau, b, nwv, B);
            }
        } else {
            for (; r < M; r += nwv) {
                const size_t ro = (size_t)b * N;
                acc.add(load_3(bq + (size_t)tau * bslab + ro), load_3(aq + (size_t)tau * gslab + ro),
                        load_3(cq + (size_t)tau * gslab + ro), load_3(sq + (size_t)tau * sslab + ro));
                advance(tau, b, nwv, B);
            }
        }
    }
    part[0][wv][lane] = acc.ad;
    part[1][wv][lane] = acc.ae;
    part[2][wv][lane] = acc.sd;
    part[3][wv][lane] = acc.se;
    __syncthreads();
    if (wv != 0 || nc <= 0) return;
    f4 tot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) tot[q] = part[q][0][lane];
    for (int w = 1; w < nwv; ++w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) tot[q] += part[q][w][lane];
    }
    // the loaded quad starts c0 - cl columns before the first owned one (0 when N == 3)
    const size_t o = (size_t)k * N + cl;
    store_owned(am + o, tot[0], nc, c0 - cl);
    store_owned(ei + o, tot[1], nc, c0 - cl);
    if (sh) store_owned(sh + o, tot[2], nc, c0 - cl);
    if (in) store_owned(in + o, tot[3], nc, c0 - cl);
}

// scores[k] / iscores[k], k = k0 + blockIdx.x, from row k of am / ei; a row of a matrix whose scale flag is set becomes
// means in place (scale bits: 1 am, 2 ei, 4 sh, 8 in)
__global__ __launch_bounds__(EP_SCORE_THREADS) void k_epistasis_score(float *am, float *ei, float *sh, float *in,
                                                                      float *__restrict__ scores, float *__restrict__ iscores,
                                                                      EpPairs held, int k0, int N, int M, int scale)
{
    __shared__ float red[2][EP_SCORE_THREADS];
    const int tid = threadIdx.x;
    const int ga = held.a[blockIdx.x], gb = held.b[blockIdx.x];
    const size_t o = (size_t)(k0 + blockIdx.x) * N;
    const double dM = (double)M;
    float accA = 0.f, accE = 0.f;
    for (int n = tid; n < N; n += EP_SCORE_THREADS) {
        const float va = am[o + n], ve = ei[o + n];
        if (n != ga && n != gb) {
            accA += va;
            accE += ve;
        }
        if (scale & 1) am[o + n] = (float)((double)va / dM);
        if (scale & 2) ei[o + n] = (float)((double)ve / dM);
        if (scale & 4) sh[o + n] = (float)((double)sh[o + n] / dM);
        if (scale & 8) in[o + n] = (float)((double)in[o + n] / dM);
    }
    red[0][tid] = accA;
    red[1][tid] = accE;
    for (int h = EP_SCORE_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
    }
    if (tid == 0) {
        scores[k0 + blockIdx.x] = (float)((double)red[0][0] / (dM * (double)(N - 2)));
        iscores[k0 + blockIdx.x] = (float)((double)red[1][0] / (dM * (double)(N - 2)));
    }
}

bool epistasis_shape_ok(int T, int K, int G, int B, int N)
{
    return T >= 2 && K >= 1 && G >= 2 && B >= 1 && N >= 3 && K <= 65535 && (long long)(T - 1) * B <= INT_MAX &&
           (long long)K * B <= INT_MAX && (long long)G * B <= INT_MAX;
}

// waves per workgroup: a function of (T, B, N) alone -- neither the device nor the number of pairs in the call may
// change the order of a sum.  A wave should have at least four rows; wide rows have many workgroups already.
int epistasis_waves(int T, int B, int N)
{
    const long long M = (long long)(T - 1) * B;
    const int cap = N > 4 * EP_TILE ? 4 : EP_MAX_WAVES;
    int W = 1;
    while (W < cap && 8 * W <= M) W *= 2;
    return W;
}

size_t ep_matrix_bytes(int K, int N) { return ((size_t)K * N * sizeof(float) + 255) / 256 * 256; }

}  // namespace

extern "C" {

size_t phx_knockout_epistasis_workspace_bytes(int T, int K, int G, int B, int N)
{
    if (!epistasis_shape_ok(T, K, G, B, N)) return 0;
    return 2 * ep_matrix_bytes(K, N);
}

int phx_knockout_epistasis(const float *base, const float *singles, const float *sol, int T, int K, int G, int B, int N,
                           const int *ia_host, const int *ib_host, const int *genes_host, float *scores,
                           float *interaction_scores, float *shift, float *magnitude, float *interaction,
                           float *interaction_magnitude, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!base || !singles || !sol || !ia_host || !ib_host || !genes_host || !scores || !interaction_scores ||
        !epistasis_shape_ok(T, K, G, B, N))
        return PHX_ERR_BAD_ARG;
    for (int g = 0; g < G; ++g)
        if (genes_host[g] < 0 || genes_host[g] >= N) return PHX_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k)
        if (ia_host[k] < 0 || ia_host[k] >= G || ib_host[k] < 0 || ib_host[k] >= G || ia_host[k] == ib_host[k])
            return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_knockout_epistasis_workspace_bytes(T, K, G, B, N)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // the |d_ab| and |e| sums: the scores need them either way
    float *am = magnitude ? magnitude : (float *)workspace;
    float *ei = interaction_magnitude ? interaction_magnitude : (float *)((char *)workspace + ep_matrix_bytes(K, N));
    const int W = epistasis_waves(T, B, N);
    const int scale = (magnitude ? 1 : 0) | (interaction_magnitude ? 2 : 0) | (shift ? 4 : 0) | (interaction ? 8 : 0);
    for (int k0 = 0; k0 < K; k0 += EP_PAIRS_PER_LAUNCH) {
        const int nk = K - k0 < EP_PAIRS_PER_LAUNCH ? K - k0 : EP_PAIRS_PER_LAUNCH;
        EpPairs idx, held;
        memset(&idx, 0, sizeof(idx));
        memset(&held, 0, sizeof(held));
        for (int i = 0; i < nk; ++i) {
            idx.a[i] = ia_host[k0 + i];
            idx.b[i] = ib_host[k0 + i];
            held.a[i] = genes_host[ia_host[k0 + i]];
            held.b[i] = genes_host[ib_host[k0 + i]];
        }
        hipLaunchKernelGGL(k_epistasis_sum, dim3((N + EP_TILE - 1) / EP_TILE, nk), dim3(W * 64), 0, st, base, singles, sol, am,
                           ei, shift, interaction, idx, k0, K, G, T, B, N);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
        hipLaunchKernelGGL(k_epistasis_score, dim3(nk), dim3(EP_SCORE_THREADS), 0, st, am, ei, shift, interaction, scores,
                           interaction_scores, held, k0, N, (T - 1) * B, scale);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}

}  // extern "C"
