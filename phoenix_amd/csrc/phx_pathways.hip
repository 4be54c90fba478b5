// phx_pathways.hip -- pathway permutation tests on one score per gene (the reference's create_permutation_test_files_aws.R):
// for every pathway p (a set of genes, CSR) and every permutation r in [first, first + n_perm) of the gene labels,
// x_r[p] = sum over the pathway's genes of the permuted scores, reduced on the fly to count = #{r : base < x_r},
// s1 = sum_r (x_r - base), s2 = sum_r (x_r - base)^2 with base[p] the sum over the scores themselves.  A permutation is a
// function of (seed, r) alone (include/phoenix_hip.h states the generator): gene g gets a 64-bit key whose low 14 bits are g,
// and the genes sorted by key are the order.  One permutation lives in LDS only; nothing of size N x n_perm exists anywhere.
//
//   grid          G = min(n_perm, 512) workgroups, a function of n_perm alone; workgroup w takes r = first + w, + G, ...
//                 (an ordinary grid: workgroups do not wait for each other, the device runs as many at once as fit).
//   permutation   keys of the genes, padded to the next power of two with all-ones words (no gene has key bits 0x3fff set in
//                 its low 14 bits unless N = 16384, where nothing is padded: pads sort last) -> bitonic sort in LDS, 8 bytes
//                 an element, 128 KiB at N = 16384 -> every position's gene is read back, its score fetched, and the float
//                 scores overwrite the front of the same LDS region.
//   walk          16 adjacent lanes share a pathway: lane l adds members l, l + 16, ... in that order in double, the 16 sums
//                 are added by a butterfly (every lane ends with the same bits).  The order is a function of the member list
//                 alone, and k_pathway_base runs the very same walk over the unpermuted scores.  The member indices are read
//                 as 16-bit words, 32 contiguous bytes per pathway and step (the entry point narrows the caller's int32 list
//                 into the workspace first).  Lane 0 of the 16 keeps the pathway's count, s1, s2 in the workgroup's row of
//                 the partials [G][P]: written by the workgroup's first permutation, read and rewritten by the later ones.
//   reduce        k_pathway_reduce, one thread per pathway, adds the G rows in row order.
//   diagnostic    PHX_DIAG=1 with PHX_PATHWAYS_STAGES=1 | 2 | 3 in the environment (read per call) ends every permutation after
//                 its keys, its sort or its score image: the results are then meaningless, the differences of the times are
//                 the stages' shares (tools/bench_pathways.py).
// No atomics: base and count are exact, s1 and s2 have an order fixed by (first, n_perm), so identical calls give identical
// bits on every device.  Lanes balance best when adjacent pathways have similar sizes (the Python caller sorts them).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "../../include/phoenix_hip.h"
#include "phx_host.hpp"

namespace {

typedef unsigned long long u64;

constexpr int PW_MAX_N = 16384;                      // a gene is 14 bits of its key; 8 B x 16384 = 128 KiB of LDS
constexpr int PW_GENE_BITS = 14;
constexpr u64 PW_GENE_MASK = (1ull << PW_GENE_BITS) - 1;
constexpr long long PW_MAX_R = 1ll << 50;            // r << 14 stays inside 64 bits
constexpr int PW_MAX_THREADS = 1024;
constexpr int PW_LANES = 16;                         // lanes that share a pathway
constexpr int PW_GROUPS = 512;                       // workgroups of a call with that many permutations or more
constexpr int PW_STAGE = PW_MAX_N / PW_MAX_THREADS;  // positions a thread carries from the key image to the score image
constexpr int PW_BASE_THREADS = 256;
enum { PW_KEYS = 1, PW_SORT = 2, PW_IMAGE = 3, PW_ALL = 4 };   // the stages of a permutation (PHX_PATHWAYS_STAGES)

__device__ __forceinline__ u64 pw_mix(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ u64 pw_key(u64 seed, u64 r, unsigned g)
{
    const u64 c = (r << PW_GENE_BITS) | g;
    return (pw_mix(pw_mix(seed + 0x9E3779B97F4A7C15ull * (c + 1))) & ~PW_GENE_MASK) | g;
}

// the sum of vals[idx[j]], j in [a, b), as the 16 lanes of a pathway form it: every lane returns the same double.  A lane
// adds its members one after the other; eight of its indices are fetched at a time so that their latencies overlap
__device__ __forceinline__ double pw_sum(const float *vals, const unsigned short *idx, long long a, long long b, int lane)
{
    constexpr int U = 8;
    double x = 0.0;
    long long j = a + lane;
    for (; j + (U - 1) * PW_LANES < b; j += U * PW_LANES) {
        unsigned short g[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) g[u] = idx[j + u * PW_LANES];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = vals[g[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) x += (double)v[u];
    }
    {
        unsigned short g[U - 1];
        float v[U - 1];
#pragma unroll
        for (int u = 0; u < U - 1; ++u) g[u] = j + u * PW_LANES < b ? idx[j + u * PW_LANES] : 0;
#pragma unroll
        for (int u = 0; u < U - 1; ++u) v[u] = vals[g[u]];
#pragma unroll
        for (int u = 0; u < U - 1; ++u)
            if (j + u * PW_LANES < b) x += (double)v[u];
    }
#pragma unroll
    for (int d = PW_LANES / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__global__ void k_pathway_narrow(const int *idx, unsigned short *idx16, long long nnz)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (long long)gridDim.x * blockDim.x)
        idx16[j] = (unsigned short)idx[j];
}

__global__ __launch_bounds__(PW_BASE_THREADS) void k_pathway_base(const float *scores, int N, const long long *ptr,
                                                                  const unsigned short *idx, int P, double *base)
{
    extern __shared__ __align__(16) unsigned char pw_lds[];
    float *vals = reinterpret_cast<float *>(pw_lds);
    for (int g = threadIdx.x; g < N; g += blockDim.x) vals[g] = scores[g];
    __syncthreads();
    const int lane = threadIdx.x % PW_LANES, per = blockDim.x / PW_LANES;
    for (long long p = (long long)blockIdx.x * per + threadIdx.x / PW_LANES; p < P; p += (long long)gridDim.x * per) {
        const double x = pw_sum(vals, idx, ptr[p], ptr[p + 1], lane);
        if (lane == 0) base[p] = x;
    }
}

__global__ __launch_bounds__(PW_MAX_THREADS) void k_pathway_perm(const float *scores, int N, int Npad, const long long *ptr,
                                                                 const unsigned short *idx, int P, u64 seed, long long first,
                                                                 long long n_perm, const double *base, long long *pcount,
                                                                 double *ps1, double *ps2, int stages)
{
    extern __shared__ __align__(16) unsigned char pw_lds[];
    u64 *keys = reinterpret_cast<u64 *>(pw_lds);            // [Npad] while a permutation is sorted
    float *vals = reinterpret_cast<float *>(pw_lds);        // [N] afterwards: the permuted scores
    const int tid = threadIdx.x, T = blockDim.x, lane = tid % PW_LANES, per = T / PW_LANES;
    const size_t row = (size_t)blockIdx.x * P;
    bool fresh = true;
    for (long long q = blockIdx.x; q < n_perm; q += gridDim.x) {
        const u64 r = (u64)(first + q);
        for (int g = tid; g < Npad; g += T) keys[g] = g < N ? pw_key(seed, r, (unsigned)g) : ~0ull;
        __syncthreads();
        if (stages < PW_SORT) continue;
        for (int k = 2; k <= Npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (Npad >> 1); t += T) {
                    const int i = 2 * t - (t & (j - 1)), l = i + j;          // bit j of i is clear
                    const u64 a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
                __syncthreads();
            }
        }
        if (stages < PW_IMAGE) continue;
        // position -> gene -> score, carried over the barrier in registers: the scores overwrite the keys
        float v[PW_STAGE];
#pragma unroll
        for (int m = 0; m < PW_STAGE; ++m) {
            const int pos = tid + m * T;
            v[m] = pos < N ? scores[(unsigned)(keys[pos] & PW_GENE_MASK)] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < PW_STAGE; ++m) {
            const int pos = tid + m * T;
            if (pos < N) vals[pos] = v[m];
        }
        __syncthreads();
        if (stages < PW_ALL) continue;
        // the pathway's bounds are fetched one pathway ahead, its partial sums before its walk: one latency, not three
        long long p = tid / PW_LANES, lo = 0, hi = 0;
        if (p < P) {
            lo = ptr[p];
            hi = ptr[p + 1];
        }
        for (; p < P; p += per) {
            const long long a = lo, b = hi;
            if (p + per < P) {
                lo = ptr[p + per];
                hi = ptr[p + per + 1];
            }
            long long c0 = 0;
            double b0 = 0.0, t1 = 0.0, t2 = 0.0;
            if (lane == 0) {
                b0 = base[p];
                if (!fresh) {
                    c0 = pcount[row + p];
                    t1 = ps1[row + p];
                    t2 = ps2[row + p];
                }
            }
            const double x = pw_sum(vals, idx, a, b, lane);
            if (lane == 0) {
                const double d = x - b0;
                pcount[row + p] = c0 + (b0 < x ? 1 : 0);
                ps1[row + p] = t1 + d;
                ps2[row + p] = t2 + d * d;
            }
        }
        fresh = false;
        __syncthreads();                                      // the next permutation's keys overwrite the scores
    }
}

__global__ void k_pathway_reduce(const long long *pcount, const double *ps1, const double *ps2, int P, int G, long long *count,
                                 double *s1, double *s2)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    long long c = 0;
    double a = 0.0, b = 0.0;
    for (int g = 0; g < G; ++g) {
        c += pcount[(size_t)g * P + p];
        a += ps1[(size_t)g * P + p];
        b += ps2[(size_t)g * P + p];
    }
    count[p] = c;
    s1[p] = a;
    s2[p] = b;
}

bool pw_shape_ok(int N, int P, long long nnz, long long n_perm)
{
    return N >= 1 && N <= PW_MAX_N && P >= 1 && nnz >= 0 && n_perm >= 1 && n_perm <= PW_MAX_R;
}

// the sort's power of two (at least 2: the compare-exchange network has no smaller form)
int pw_padded(int N)
{
    int n = 2;
    while (n < N) n <<= 1;
    return n;
}

// one thread per compare-exchange of a sort step, whole waves, at most 1024; PW_STAGE positions per thread cover Npad then
int pw_threads(int Npad)
{
    const int t = Npad / 2;
    return t < 64 ? 64 : t > PW_MAX_THREADS ? PW_MAX_THREADS : t;
}

int pw_groups(long long n_perm) { return n_perm < PW_GROUPS ? (int)n_perm : PW_GROUPS; }

// diagnostic builds of a timing only: honoured together with PHX_DIAG=1, as PHX_LIB is
int pw_stages()
{
    const char *d = getenv("PHX_DIAG"), *e = getenv("PHX_PATHWAYS_STAGES");
    if (!d || strcmp(d, "1") != 0 || !e) return PW_ALL;
    const int v = atoi(e);
    return v >= PW_KEYS && v < PW_ALL ? v : PW_ALL;
}

struct pw_layout {
    size_t idx16, cnt, s1, s2, total;
};

pw_layout pw_workspace(int P, long long nnz, int G)
{
    phxh::Take take;
    pw_layout w;
    w.idx16 = take((size_t)nnz * sizeof(unsigned short));
    w.cnt = take((size_t)G * P * sizeof(long long));
    w.s1 = take((size_t)G * P * sizeof(double));
    w.s2 = take((size_t)G * P * sizeof(double));
    w.total = take.off;
    return w;
}

}  // namespace

extern "C" {

size_t phx_pathway_permutations_workspace_bytes(int N, int P, long long nnz, long long n_perm)
{
    if (!pw_shape_ok(N, P, nnz, n_perm)) return 0;
    return pw_workspace(P, nnz, pw_groups(n_perm)).total;
}

int phx_pathway_permutations(const float *scores, int N, const long long *ptr, const int *idx, int P, long long nnz,
                             unsigned long long seed, long long first, long long n_perm, double *base, long long *count,
                             double *s1, double *s2, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pw_shape_ok(N, P, nnz, n_perm)) return PHX_ERR_BAD_ARG;
    if (first < 0 || first > PW_MAX_R - n_perm) return PHX_ERR_BAD_ARG;
    if (!scores || !ptr || (!idx && nnz > 0) || !base || !count || !s1 || !s2) return PHX_ERR_BAD_ARG;
    const int G = pw_groups(n_perm);
    const pw_layout w = pw_workspace(P, nnz, G);
    if (!workspace || workspace_bytes < w.total) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    unsigned short *idx16 = reinterpret_cast<unsigned short *>(ws + w.idx16);
    long long *pcount = reinterpret_cast<long long *>(ws + w.cnt);
    double *ps1 = reinterpret_cast<double *>(ws + w.s1), *ps2 = reinterpret_cast<double *>(ws + w.s2);
    if (nnz > 0) {
        const long long blocks = (nnz + 255) / 256;
        hipLaunchKernelGGL(k_pathway_narrow, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, idx, idx16, nnz);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    }
    {
        const size_t lds = (size_t)N * sizeof(float);
        if (!phxh::set_lds(k_pathway_base, lds)) return PHX_ERR_LAUNCH;
        const int per = PW_BASE_THREADS / PW_LANES, blocks = (P + per - 1) / per;
        hipLaunchKernelGGL(k_pathway_base, dim3(blocks < 1024 ? blocks : 1024), dim3(PW_BASE_THREADS), lds, st, scores, N, ptr,
                           idx16, P, base);
        if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    }
    const int Npad = pw_padded(N);
    const size_t lds = (size_t)Npad * sizeof(u64);
    if (!phxh::set_lds(k_pathway_perm, lds)) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL(k_pathway_perm, dim3(G), dim3(pw_threads(Npad)), lds, st, scores, N, Npad, ptr, idx16, P, (u64)seed, first,
                       n_perm, base, pcount, ps1, ps2, pw_stages());
    if (hipGetLastError() != hipSuccess) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL(k_pathway_reduce, dim3((P + 255) / 256), dim3(256), 0, st, pcount, ps1, ps2, P, G, count, s1, s2);
    return hipGetLastError() == hipSuccess ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // extern "C"
