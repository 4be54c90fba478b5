// phx_hillko.hip -- knockout screens of the ground-truth Hill-kinetics simulator (phx_hill.inc): K calls of the same B
// samples, call k with gene genes[k] HELD at values[k] (its column starts at the level and its rate is 0 in every stage),
// genes[k] == -1 the unperturbed call.  The truth that analysis.knockout_effects (the model's screen: phx_odeint_clamped)
// is scored against, in the sol layout of phx_knockout_effects: row k * B + b of every time slice belongs to call k.
//
// k_hill_simulate interprets one postfix program per thread: the 64 lanes of a wave walk 64 different programs, so most of
// an interpreter step is fetch, decode and divergence, not arithmetic.  The calls of a screen integrate the same sample
// under the same programs, so here a thread fetches and decodes an instruction ONCE and applies it to the operand stacks
// of KPT calls:
//
//   group         One workgroup integrates KPT calls of one sample (slots j < KPT = calls k0 + j of the launch); their KPT
//                 states sit in LDS, slot-major ([KPT][N] floats).  Thread t owns genes t, t + nt, ... (GPT of them), as
//                 in k_hill_simulate; y / acc / k of its GPT x KPT (gene, slot) pairs are registers.
//   interpreter   hill_eval_slots: the program of a gene is walked once per stage; every instruction runs on the KPT
//                 stacks.  The top of a stack is a register, the elements below it sit in a runtime-indexed array (scratch):
//                 a push only stores, a binary operation loads once.  The KPT dependency chains are independent, so the
//                 latency of one scratch access is shared by KPT calls.  The operations and their order are hill_eval's.
//   integrator    k_hill_simulate's: classical RK4, nsub = max(1, ceil(|span| / dt_max)) equal sub-steps per interval,
//                 h = (float)(span / nsub), fp32 state, fAct continued by 0 at TF <= 0.
//   clamp         The rate of (gene genes[k], slot of call k) is replaced by 0 after the evaluation: y + h * 0 = y exactly,
//                 in every stage and in the final sum, so the column holds its level bit for bit.
//   no remainder  There is one instantiation per (KPT, GPT) and NO remainder path: a slot without a call (the last group
//                 of a launch) integrates the unperturbed system and stores nothing.  The arithmetic of a slot does not
//                 look at the other slots, at its slot index or at the group: the bits of call k are the same alone, first
//                 or last in a group, beside a duplicate of itself, in a remainder group.  A gene the clamped gene cannot
//                 reach therefore has a shift of exactly 0 against the -1 call.
//   budget        GPT = 1, 2, 4, 8 genes per thread (N <= 1024 GPT); KPT x GPT <= 8 keeps the 3 KPT GPT state registers
//                 of a thread at 24, those of k_hill_simulate (1024 threads leave 128 VGPRs each), and the LDS of a group
//                 at KPT N floats <= 32 KiB: several groups per CU at every N, no raised dynamic-LDS limit.  The stacks
//                 are 24 KPT floats of scratch per thread.  KPT <= HK_KPT_SHIPPED: profiles/hill_knockouts.json
//                 (tools/bench_hill_knockouts.py) has the measured times of every KPT.
//   launches      Clamped genes and levels travel as launch arguments, HK_CALLS_PER_LAUNCH calls per launch (2 KiB).
//                 Groups are strided over a capped gridDim.x and rows over a capped gridDim.y: neither K nor B is bounded
//                 by a grid dimension.  Nothing allocates, copies or synchronises.
//   sets          phx_hill_knockout_sets: a call holds a SET of up to PHX_HILL_HOLD_MAX genes, each at its own level (pair
//                 and higher-order knockouts).  The width W of a slot's row of held genes is a template parameter of the
//                 same kernel -- W = 1 is phx_hill_knockouts, instruction for instruction -- and the only difference is
//                 the clamp test, "gene is one of the W entries of the slot's row" (-1 pads a shorter set and matches no
//                 gene).  W = 1, 2, 4 are instantiated, a width of 3 runs padded at W = 4.  The launch arguments stay at
//                 2 KiB: HK_CALLS_PER_LAUNCH / W calls per launch.  The arithmetic of a (gene, slot) that is not held does
//                 not look at W: a call's bits are the same at every width its set fits in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/phoenix_hip.h"

#include "phx_hill.inc"

namespace {

constexpr int HK_CALLS_PER_LAUNCH = 256;   // genes and levels of a launch: 2 KiB of kernel arguments
constexpr int HK_MAX_GRID_X = 4096;        // groups of a launch are strided over gridDim.x
constexpr int HK_MAX_GRID_Y = 4096;        // rows are strided over gridDim.y
constexpr int HK_SLOT_BUDGET = 8;          // KPT x GPT (see `budget` above)
constexpr int HK_KPT_SHIPPED = 2;          // the KPT that measured fastest on the shipped 350-gene screen

// the held genes and levels of a launch, HK_CALLS_PER_LAUNCH / W rows of W entries (-1: no gene): 2 KiB at every W
template <int W>
struct HkCalls {
    static constexpr int CALLS = HK_CALLS_PER_LAUNCH / W;
    int g[CALLS * W];
    float v[CALLS * W];
};

// hill_eval on KPT states at once: xs [KPT][N], res[j] = the rate of `gene` at state j
template <int KPT>
__device__ __forceinline__ void hill_eval_slots(const HillProg &p, int gene, const float *xs, int N, float (&res)[KPT])
{
    // element i of a stack of n elements: i == n - 1 in top[], i < n - 1 in st[i + 1] (st[0] takes the first push's idle top)
    float st[HILL_STACK][KPT], top[KPT];
    int n = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) top[j] = 0.f;
    const int2 *c = p.code + p.off[gene];
    const int len = p.len[gene];
    for (int i = 0; i < len; ++i) {
        const int2 ins = c[i];
        switch (ins.x) {
            case HOP_PUSHC: {
                const float cst = p.consts[ins.y];
#pragma unroll
                for (int j = 0; j < KPT; ++j) { st[n][j] = top[j]; top[j] = cst; }
                n++;
                break;
            }
            case HOP_PUSHX:
#pragma unroll
                for (int j = 0; j < KPT; ++j) { st[n][j] = top[j]; top[j] = xs[j * N + ins.y]; }
                n++;
                break;
            case HOP_ADD:
                n--;
#pragma unroll
                for (int j = 0; j < KPT; ++j) top[j] = st[n][j] + top[j];
                break;
            case HOP_SUB:
                n--;
#pragma unroll
                for (int j = 0; j < KPT; ++j) top[j] = st[n][j] - top[j];
                break;
            case HOP_MUL:
                n--;
#pragma unroll
                for (int j = 0; j < KPT; ++j) top[j] = st[n][j] * top[j];
                break;
            case HOP_DIV:
                n--;
#pragma unroll
                for (int j = 0; j < KPT; ++j) top[j] = st[n][j] / top[j];
                break;
            case HOP_NEG:
#pragma unroll
                for (int j = 0; j < KPT; ++j) top[j] = -top[j];
                break;
            default: {   // HOP_FACT
                const float B = p.consts[ins.y], K = p.consts[ins.y + 1], nn = p.consts[ins.y + 2];
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    const float tf = top[j];
                    const float tn = tf > 0.f ? powf(tf, nn) : 0.f;
                    top[j] = B * tn / (K + tn);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j) res[j] = len > 0 ? top[j] : 0.f;
}

// is `gene` one of the W held genes of a slot
template <int W>
__device__ __forceinline__ bool hk_held(int gene, const int (&cg)[W])
{
    bool held = gene == cg[0];
#pragma unroll
    for (int w = 1; w < W; ++w) held = held || gene == cg[w];
    return held;
}

// calls k0 .. k0 + nk - 1 of the screen (k0: the first call of this launch), out [T, K * B, N]
template <int KPT, int GPT, int W>
__global__ __launch_bounds__(1024) void k_hill_knockouts(HillProg p, const float *__restrict__ x0,
                                                         const double *__restrict__ times, int T, double dt_max,
                                                         HkCalls<W> calls, int k0, int nk, int K, float *__restrict__ out,
                                                         int B, int N)
{
    extern __shared__ float xs[];   // [KPT][N]
    const int tid = threadIdx.x, nt = blockDim.x;
    const int ngroups = (nk + KPT - 1) / KPT;
    const long long slab = (long long)K * B * N;   // floats of one output time
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
            int cg[KPT][W];     // the clamped genes of slot j (-1: none)
            float cv[KPT][W];
            bool live[KPT];     // the slot has a call: its states are stored
            float *orow[KPT];   // out[0, k * B + b, 0]
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const int kl = grp * KPT + j;
                live[j] = kl < nk;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    cg[j][w] = live[j] ? calls.g[kl * W + w] : -1;
                    cv[j][w] = live[j] ? calls.v[kl * W + w] : 0.f;
                }
                orow[j] = out + ((long long)(k0 + (live[j] ? kl : 0)) * B + b) * N;
            }
            float y[GPT][KPT], acc[GPT][KPT], k[GPT][KPT];
#pragma unroll
            for (int g = 0; g < GPT; ++g) {
                const int gene = tid + g * nt;
                const float v0 = gene < N ? x0[(long long)b * N + gene] : 0.f;
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    y[g][j] = v0;
#pragma unroll
                    for (int w = 0; w < W; ++w) y[g][j] = gene == cg[j][w] ? cv[j][w] : y[g][j];
                    if (gene < N) {
                        xs[j * N + gene] = y[g][j];
                        if (live[j]) orow[j][gene] = y[g][j];
                    }
                }
            }
            __syncthreads();
            auto stage = [&](float wk, float hnext, bool last) {   // k = f(xs); acc += wk k; xs = y + hnext k (or new y)
#pragma unroll
                for (int g = 0; g < GPT; ++g) {
                    const int gene = tid + g * nt;
                    if (gene < N) {
                        hill_eval_slots<KPT>(p, gene, xs, N, k[g]);
                    } else {
#pragma unroll
                        for (int j = 0; j < KPT; ++j) k[g][j] = 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < KPT; ++j) {
                        if (hk_held<W>(gene, cg[j])) k[g][j] = 0.f;   // the clamp: rate 0 in every stage
                        acc[g][j] += wk * k[g][j];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int g = 0; g < GPT; ++g) {
                    const int gene = tid + g * nt;
#pragma unroll
                    for (int j = 0; j < KPT; ++j) {
                        if (last) y[g][j] = y[g][j] + hnext * acc[g][j];
                        if (gene < N) xs[j * N + gene] = last ? y[g][j] : y[g][j] + hnext * k[g][j];
                    }
                }
                __syncthreads();
            };
            for (int i = 0; i + 1 < T; ++i) {
                const double span = times[i + 1] - times[i];
                const int nsub = max(1, (int)ceil(fabs(span) / dt_max));
                const float h = (float)(span / nsub);
                for (int s = 0; s < nsub; ++s) {
#pragma unroll
                    for (int g = 0; g < GPT; ++g)
#pragma unroll
                        for (int j = 0; j < KPT; ++j) acc[g][j] = 0.f;
                    stage(1.f, 0.5f * h, false);
                    stage(2.f, 0.5f * h, false);
                    stage(2.f, h, false);
                    stage(1.f, h / 6.f, true);
                }
#pragma unroll
                for (int g = 0; g < GPT; ++g) {
                    const int gene = tid + g * nt;
#pragma unroll
                    for (int j = 0; j < KPT; ++j)
                        if (gene < N && live[j]) orow[j][(long long)(i + 1) * slab + gene] = y[g][j];
                }
            }
            // the last stage ended in a barrier (T == 1: the one after the initial stores): xs is free for the next group
        }
    }
}

int hillko_gpt(int N) { return N <= 1024 ? 1 : N <= 2048 ? 2 : N <= 4096 ? 4 : 8; }

// calls per workgroup at N genes: the shipped KPT where the slot budget has room for it; PHX_HILLKO_KPT = 1 | 2 | 4 | 8
// asks for another one (the timing tool walks them), cut to the budget in the same way
int hillko_kpt(int N)
{
    int want = HK_KPT_SHIPPED;
    const char *e = getenv("PHX_HILLKO_KPT");
    if (e && (e[0] == '1' || e[0] == '2' || e[0] == '4' || e[0] == '8') && e[1] == 0) want = e[0] - '0';
    const int room = HK_SLOT_BUDGET / hillko_gpt(N);
    return want < room ? want : room;
}

template <int KPT, int GPT, int W>
hipError_t hillko_launch(dim3 grid, int threads, hipStream_t st, const HillProg &p, const float *x0, const double *times, int T,
                         double dt_max, const HkCalls<W> &c, int k0, int nk, int K, float *out, int B, int N)
{
    hipLaunchKernelGGL((k_hill_knockouts<KPT, GPT, W>), grid, dim3(threads), sizeof(float) * (size_t)KPT * (size_t)N, st, p,
                       x0, times, T, dt_max, c, k0, nk, K, out, B, N);
    return hipGetLastError();
}

// what both entry points refuse besides their lists
bool hillko_bad_shape(const void *code, const void *off, const void *len, const void *consts, const void *x0, const void *times,
                      const void *genes_host, const void *values_host, const void *out, int T, double dt_max, int K, int B, int N)
{
    return !code || !off || !len || !consts || !x0 || !times || !genes_host || !values_host || !out || B < 1 || N < 1 || K < 1 ||
           T < 1 || !(dt_max > 0.0) || N > HILL_GPT * 1024 || (long long)K * B > INT_MAX;
}

// the launches of a checked screen whose rows genes_host / values_host [K][width] fit W entries (width <= W: -1 pads)
template <int W>
int hillko_run(const HillProg &p, const float *x0, const double *times, int T, double dt_max, const int *genes_host,
               const float *values_host, int width, int K, float *out, int B, int N, hipStream_t st)
{
    constexpr int CALLS = HkCalls<W>::CALLS;
    const int gpt = hillko_gpt(N), kpt = hillko_kpt(N);
    const int per = (N + gpt - 1) / gpt;   // genes per slot of a thread's list: N <= gpt * threads
    const int threads = std::min(1024, ((per + 63) / 64) * 64);
    for (int k0 = 0; k0 < K; k0 += CALLS) {
        const int nk = K - k0 < CALLS ? K - k0 : CALLS;
        HkCalls<W> c;
        memset(&c, 0, sizeof(c));
        for (int k = 0; k < nk; ++k)
            for (int w = 0; w < W; ++w) {
                const int g = w < width ? genes_host[(size_t)(k0 + k) * width + w] : -1;
                c.g[k * W + w] = g;
                c.v[k * W + w] = g >= 0 ? values_host[(size_t)(k0 + k) * width + w] : 0.f;   // the level of a pad is ignored
            }
        const int ngroups = (nk + kpt - 1) / kpt;
        const dim3 grid(ngroups < HK_MAX_GRID_X ? ngroups : HK_MAX_GRID_X, B < HK_MAX_GRID_Y ? B : HK_MAX_GRID_Y);
        hipError_t e = hipErrorInvalidValue;
#define HK_CASE(KPT_, GPT_) \
    if (kpt == KPT_ && gpt == GPT_) \
        e = hillko_launch<KPT_, GPT_, W>(grid, threads, st, p, x0, times, T, dt_max, c, k0, nk, K, out, B, N)
        HK_CASE(1, 1); HK_CASE(2, 1); HK_CASE(4, 1); HK_CASE(8, 1);
        HK_CASE(1, 2); HK_CASE(2, 2); HK_CASE(4, 2);
        HK_CASE(1, 4); HK_CASE(2, 4);
        HK_CASE(1, 8);
#undef HK_CASE
        if (e != hipSuccess) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}

}  // namespace

extern "C" {

int phx_debug_hill_knockouts_kpt(int N) { return N >= 1 && N <= HILL_GPT * 1024 ? hillko_kpt(N) : 0; }

int phx_hill_knockouts(const int *code, const int *off, const int *len, const float *consts, const float *x0,
                       const double *times, int T, double dt_max, const int *genes_host, const float *values_host, int K,
                       float *out, int B, int N, void *stream)
{
    if (hillko_bad_shape(code, off, len, consts, x0, times, genes_host, values_host, out, T, dt_max, K, B, N))
        return PHX_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k)
        if (genes_host[k] < -1 || genes_host[k] >= N || !std::isfinite(values_host[k])) return PHX_ERR_BAD_ARG;
    const HillProg p{reinterpret_cast<const int2 *>(code), off, len, consts};
    return hillko_run<1>(p, x0, times, T, dt_max, genes_host, values_host, 1, K, out, B, N, (hipStream_t)stream);
}

int phx_hill_knockout_sets(const int *code, const int *off, const int *len, const float *consts, const float *x0,
                           const double *times, int T, double dt_max, const int *genes_host, const float *values_host,
                           int width, int K, float *out, int B, int N, void *stream)
{
    if (hillko_bad_shape(code, off, len, consts, x0, times, genes_host, values_host, out, T, dt_max, K, B, N) || width < 1 ||
        width > PHX_HILL_HOLD_MAX)
        return PHX_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k) {
        const int *row = genes_host + (size_t)k * width;
        for (int w = 0; w < width; ++w) {
            if (row[w] < -1 || row[w] >= N) return PHX_ERR_BAD_ARG;
            if (row[w] < 0) continue;   // a pad: its level is not looked at
            if (!std::isfinite(values_host[(size_t)k * width + w])) return PHX_ERR_BAD_ARG;
            for (int u = 0; u < w; ++u)
                if (row[u] == row[w]) return PHX_ERR_BAD_ARG;   // a gene twice: two levels would be ambiguous
        }
    }
    const HillProg p{reinterpret_cast<const int2 *>(code), off, len, consts};
    hipStream_t st = (hipStream_t)stream;
    if (width == 1) return hillko_run<1>(p, x0, times, T, dt_max, genes_host, values_host, width, K, out, B, N, st);
    if (width == 2) return hillko_run<2>(p, x0, times, T, dt_max, genes_host, values_host, width, K, out, B, N, st);
    return hillko_run<4>(p, x0, times, T, dt_max, genes_host, values_host, width, K, out, B, N, st);
}

}  // extern "C"
