// phx_steady.hip -- what the steady-state solve (phoenix_amd.steady_states) needs on the device.
//
// On the genes that move, f(y) = relu(g) (Wa h(y) - y) with h(y) = [Ws a(y) + bs ; exp(Wp l(y) + bp)], so the Jacobian is a
// diagonal plus a product through the 2H-wide hidden vector, and a linearly implicit step of weights m (per gene) is
//     delta = m (r + Wa x),   (I - S) x = w,   S = C(y) diag(m) Wa,   w = C(y) (m r),   r = Wa h(y) - y
// with C(y) = [Ws diag(a'(y)) ; diag(v) Wp diag(l'(y))] and v = exp(Wp l(y) + bp).
//
//   k_rj          S, w and the hidden vector of a state are contractions over the genes with the same A operands, the rows of
//                 Ws (sums branch) and of Wp (products branch); the B operand is the N x (2H + 2) block
//                 [diag(d m) WaT^T | act | d m r] with (act, d) = (a, a') or (l, l').  A workgroup (256 threads, four waves
//                 of 32 x 32 outputs) owns a 64 x 64 block of one branch's H x (2H + 2) outputs, a segment of the gene axis
//                 and a group of RJ_SB = 4 states.  It walks its segment TILE_KC = 32 genes at a time: the chunk's 64 rows of
//                 the branch's weights and 64 rows of WaT lie in LDS (the row-major panels of phx_steady_tile.inc, which
//                 holds what the tile kernels of the family share) and stay there while the workgroup walks its states;
//                 the state's three per-gene vectors lie beside them, and the B operand is the WaT entry times the vector
//                 of the lane's column (the last two columns hold 1.0 in the panel), formed as it is read.
//                 v_mfma_f32_16x16x4_f32, K ascending.  A 16 x 16 tile outside the matrix is not computed.
//   k_rj_finish   adds the segments' partial blocks in segment order, adds the bias (and takes exp) for the hidden vector,
//                 and scales the product rows of S and w by v_j afterwards.
//   sum order     entry (j, c) of a state: per segment the fmaf chain of the MFMA over the segment's genes ascending (four
//                 lanes' chains of every fourth gene, added by the instruction in a fixed order), then the S partials
//                 ascending.  The segments are a function of (N, H) alone, and a state shares its accumulators with no
//                 other: its bits depend neither on B nor on the other states of the call.  No atomics.
//   k_st_hidden, k_st_wa, k_st_solve   the RHS-sized passes and the dense solve of the iteration, each in an order fixed by
//                 the shape alone: the hidden vector of a state (one workgroup per four hidden rows), out = x WaT with the
//                 residual or the update fused (c ascending, one thread per gene), and (I - S) x = w in double by LU with
//                 partial pivoting, one workgroup per state, by the rule and the steps that phx_dense_lu.inc describes
//                 (k_sr_inverse, phx_steady_resp.hip, calls them; this kernel keeps them written out, see there).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/phoenix_hip.h"
#include "phx_device.hpp"
#include "phx_host.hpp"

namespace {

#include "phx_dense_lu.inc"
#include "phx_steady_tile.inc"

constexpr int RJ_SB = 4;              // states of a workgroup
constexpr int RJ_WGS = 256;           // workgroups of one group of states that the segment count aims at
constexpr size_t RJ_WS_CAP = (size_t)64 << 20;   // bytes of partial blocks per launch: more states are walked in chunks
constexpr int ST_ROWS = 4;            // hidden rows of a workgroup of k_st_hidden
constexpr int LU_THREADS = 1024;      // threads of a workgroup of k_st_solve

struct rj_geom {
    int RB, CB, nblk, NC, T, S;
};

__host__ __device__ inline rj_geom rj_geometry(int N, int H)
{
    rj_geom q;
    q.NC = 2 * H + 2;
    q.RB = (H + TILE - 1) / TILE;
    q.CB = (q.NC + TILE - 1) / TILE;
    q.nblk = 2 * q.RB * q.CB;
    q.T = (N + TILE_KC - 1) / TILE_KC;
    const int want = (RJ_WGS + q.nblk - 1) / q.nblk;
    q.S = want < q.T ? want : q.T;
    return q;
}

struct rj_args {
    const float *y, *m, *r;   // [B][N]; r may be null
    float *part;              // [S][B][2H][NC]
    int B;
};

// acc[ti][tj] += A(rows of tile ti) x B(columns of tile tj) over the chunk; NI, NJ: the wave's tiles inside the matrix.
// Not tile_kloop: the B operand is scaled by the state's vector as it is read, and the tile counts are template arguments
// because the loop runs once per state of the group on the same staged chunk.
template <int NI, int NJ>
__device__ __forceinline__ void rj_kloop(const float *pa, const float *pb, const float *v0, const float *v1, f4 (&acc)[2][2])
{
#pragma unroll
    for (int kk = 0; kk < TILE_KC / 4; ++kk) {
        float a[2], b[2];
#pragma unroll
        for (int ti = 0; ti < NI; ++ti) a[ti] = pa[ti * 16 * TILE_LD + 4 * kk];
        b[0] = pb[4 * kk] * v0[4 * kk];
        if (NJ > 1) b[1] = pb[16 * TILE_LD + 4 * kk] * v1[4 * kk];
#pragma unroll
        for (int ti = 0; ti < NI; ++ti)
#pragma unroll
            for (int tj = 0; tj < NJ; ++tj) acc[ti][tj] = mfma4(a[ti], b[tj], acc[ti][tj]);
    }
}

__global__ __launch_bounds__(ST_THREADS) void k_rj(const float *__restrict__ Ws, const float *__restrict__ Wp,
                                                   const float *__restrict__ WaT, int N, int H, rj_args a)
{
    __shared__ float pa_s[TILE * TILE_LD], pb_s[TILE * TILE_LD], vec[RJ_SB * 3 * TILE_KC];
    const tile_lane L = tile_lanes();
    const int tid = L.tid;
    const rj_geom q = rj_geometry(N, H);
    const int blk = blockIdx.x % q.nblk, rest = blockIdx.x / q.nblk;
    const int seg = rest % q.S, sg = rest / q.S;
    const int br = blk / (q.RB * q.CB), rb = (blk - br * q.RB * q.CB) / q.CB, cb = blk % q.CB;
    const int row0 = rb * TILE, col0 = cb * TILE, H2 = 2 * H;
    const float *W = br ? Wp : Ws;
    const int b0 = sg * RJ_SB, nb = min(RJ_SB, a.B - b0);
    int t_begin, t_end;
    seg_range(seg, q.T, q.S, t_begin, t_end);
    const int ni = tiles_inside(H, row0 + L.iw), nj = tiles_inside(q.NC, col0 + L.jw);
    // which of the state's vectors scales this lane's column of tile tj: d m, act (column 2H) or d m r (column 2H + 1)
    int which[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int c = col0 + L.jw + 16 * tj + L.lc;
        which[tj] = c < H2 ? 0 : (c == H2 ? 1 : 2);
    }
    const float *pa = pa_s + (L.iw + L.lc) * TILE_LD + L.lq, *pb = pb_s + (L.jw + L.lc) * TILE_LD + L.lq;

    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 acc[RJ_SB][2][2];
#pragma unroll
    for (int st = 0; st < RJ_SB; ++st)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) acc[st][ti][tj] = zero;

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TILE_KC;
        __syncthreads();                       // every wave is done with the previous chunk
        // the panels: 64 rows of 32 genes each, a quad of genes per thread and step; zeros outside the matrices
#pragma unroll
        for (int u = 0; u < 2 * TILE * TILE_KC / 4 / ST_THREADS; ++u) {
            const tile_quad s = tile_quad_at(tid + u * ST_THREADS);
            const int n = n0 + s.c4, row = (s.panel ? col0 : row0) + s.rr;
            const float *src = nullptr;
            if (s.panel == 0) {
                if (row < H) src = W + (size_t)row * N + n;
            } else if (row < H2) {
                src = WaT + (size_t)row * N + n;
            }
            f4 v = ld4(src, src ? N - n : 0);          // n may lie past the row's end: ld4 reads nothing where nv <= 0
            if (s.panel == 1 && row >= H2 && row < q.NC) {          // the columns of act and of d m r
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < N) v[e] = 1.f;
            }
            st4((s.panel ? pb_s : pa_s) + s.rr * TILE_LD + s.c4, v);
        }
        // the states' vectors of the chunk: thread (st, kk)
        if (tid < RJ_SB * TILE_KC) {
            const int st = tid >> 5, kk = tid & 31, n = n0 + kk;
            float dm = 0.f, av = 0.f, dmr = 0.f;
            if (st < nb && n < N) {
                const size_t at = (size_t)(b0 + st) * N + n;
                const float yv = a.y[at], mv = a.m[at];
                float aa, ll, da, dl;
                phx::act_pair(yv, aa, ll);
                phx::act_grad(yv, da, dl);
                av = br ? ll : aa;
                if (mv != 0.f) {               // a gene of weight 0 takes no part, whatever its state and residual hold
                    dm = (br ? dl : da) * mv;
                    if (a.r) dmr = dm * a.r[at];
                }
            }
            vec[(st * 3 + 0) * TILE_KC + kk] = dm;
            vec[(st * 3 + 1) * TILE_KC + kk] = av;
            vec[(st * 3 + 2) * TILE_KC + kk] = dmr;
        }
        __syncthreads();
        if (ni > 0 && nj > 0) {
#pragma unroll
            for (int st = 0; st < RJ_SB; ++st) {
                if (st < nb) {
                    const float *v0 = vec + (st * 3 + which[0]) * TILE_KC + L.lq, *v1 = vec + (st * 3 + which[1]) * TILE_KC + L.lq;
                    if (ni == 2 && nj == 2) rj_kloop<2, 2>(pa, pb, v0, v1, acc[st]);
                    else if (ni == 2) rj_kloop<2, 1>(pa, pb, v0, v1, acc[st]);
                    else if (nj == 2) rj_kloop<1, 2>(pa, pb, v0, v1, acc[st]);
                    else rj_kloop<1, 1>(pa, pb, v0, v1, acc[st]);
                }
            }
        }
    }

    // the partial block of (segment, state): rows of the branch, NC columns
#pragma unroll
    for (int st = 0; st < RJ_SB; ++st) {
        if (st >= nb) break;
        float *out = a.part + (((size_t)seg * a.B + b0 + st) * H2 + (size_t)br * H) * q.NC;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const int c = col0 + L.jw + 16 * tj + L.lc;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + L.iw + 16 * ti + 4 * L.lq + r;
                    if (row < H && c < q.NC) out[(size_t)row * q.NC + c] = acc[st][ti][tj][r];
                }
            }
    }
}

// one workgroup per (state, hidden row j): the S partials of every column in segment order, the bias and exp of the hidden
// vector, the product rows scaled by v_j
__global__ __launch_bounds__(128) void k_rj_finish(const float *__restrict__ part, const float *__restrict__ bs,
                                                   const float *__restrict__ bp, int H, int NC, int S, int B, float *__restrict__ Sout,
                                                   float *__restrict__ w, float *__restrict__ hid)
{
    const int H2 = 2 * H, b = blockIdx.x / H2, j = blockIdx.x - b * H2;
    const size_t stride = (size_t)B * H2 * NC;
    const float *base = part + ((size_t)b * H2 + j) * NC;
    const float hs = seg_sum(base + H2, S, stride);
    const bool prod = j >= H;
    const float hv = prod ? expf(hs + bp[j - H]) : hs + bs[j];
    for (int c = threadIdx.x; c < H2; c += 128) {
        const float s = seg_sum(base + c, S, stride);
        Sout[((size_t)b * H2 + j) * H2 + c] = prod ? hv * s : s;
    }
    if (threadIdx.x == 0) {
        hid[(size_t)b * H2 + j] = hv;
        if (w) {
            const float s = seg_sum(base + H2 + 1, S, stride);
            w[(size_t)b * H2 + j] = prod ? hv * s : s;
        }
    }
}

// hid[b, j] of ST_ROWS hidden rows of one state: thread t takes genes t, t + 256, ... ascending, the wave adds by
// butterfly, the four waves in wave order
__global__ __launch_bounds__(ST_THREADS) void k_st_hidden(const float *__restrict__ Ws, const float *__restrict__ bs,
                                                          const float *__restrict__ Wp, const float *__restrict__ bp, int N, int H,
                                                          const float *__restrict__ y, float *__restrict__ hid)
{
    __shared__ float red[ST_ROWS][ST_THREADS / 64];
    const int b = blockIdx.y, j0 = blockIdx.x * ST_ROWS, H2 = 2 * H, tid = threadIdx.x;
    const float *rows[ST_ROWS];
    bool prod[ST_ROWS];
#pragma unroll
    for (int u = 0; u < ST_ROWS; ++u) {
        const int j = min(j0 + u, H2 - 1);     // a row past the end repeats the last one and is not stored
        prod[u] = j >= H;
        rows[u] = prod[u] ? Wp + (size_t)(j - H) * N : Ws + (size_t)j * N;
    }
    float acc[ST_ROWS] = {0.f, 0.f, 0.f, 0.f};
    for (int n = tid; n < N; n += ST_THREADS) {
        float aa, ll;
        phx::act_pair(y[(size_t)b * N + n], aa, ll);
#pragma unroll
        for (int u = 0; u < ST_ROWS; ++u) acc[u] = fmaf(rows[u][n], prod[u] ? ll : aa, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < ST_ROWS; ++u) {
        const float s = phx::wave_sum(acc[u]);
        if ((tid & 63) == 0) red[u][tid >> 6] = s;
    }
    __syncthreads();
    if (tid < ST_ROWS && j0 + tid < H2) {
        const int j = j0 + tid;
        const float s = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
        hid[(size_t)b * H2 + j] = j >= H ? expf(s + bp[j - H]) : s + bs[j];
    }
}

// z[b, n] = sum over c ascending of WaT[c, n] x[b, c];  update == 0: out = z - y (the residual r);  update == 1:
// out = y + m (r + z) where m != 0, y where m == 0 (a gene that does not move keeps its bits)
__global__ __launch_bounds__(ST_THREADS) void k_st_wa(const float *__restrict__ WaT, int N, int H2, const float *__restrict__ x,
                                                      const float *__restrict__ y, const float *__restrict__ m,
                                                      const float *__restrict__ r, int update, float *__restrict__ out)
{
    __shared__ float xs[2 * STEADY_MAX_H];
    const int b = blockIdx.y, n = blockIdx.x * ST_THREADS + threadIdx.x;
    for (int c = threadIdx.x; c < H2; c += ST_THREADS) xs[c] = x[(size_t)b * H2 + c];
    __syncthreads();
    if (n >= N) return;
    const size_t at = (size_t)b * N + n;
    const float yv = y[at];
    if (update && m[at] == 0.f) {
        out[at] = yv;
        return;
    }
    float z = 0.f;
    for (int c = 0; c < H2; ++c) z = fmaf(WaT[(size_t)c * N + n], xs[c], z);
    out[at] = update ? fmaf(m[at], r[at] + z, yv) : z - yv;
}

// (I - S_b) x = w_b in double, LU with partial pivoting (the first row of the largest magnitude), one workgroup of sixteen
// waves per state; A [B][n][n] doubles of workspace.  info[b] = 0, or k + 1 where column k has no finite non-zero pivot, or
// -1 where the solution is not finite as float (an entry beyond the float range counts, as the result is stored as
// float); x of such a state is zero.  Every entry is updated by one thread in an order fixed by n alone.
// The steps are written out here, not called from phx_dense_lu.inc: in one timing of whole-kernel builds (24 states,
// n = 400) every build that called one or more of the shared steps ran 0.15 % to 0.6 % slower, this one 0.07 %, against a
// spread of 0.1 % between runs.  That is no cost of a single step.  A change of the pivot rule is made here and there.
__global__ __launch_bounds__(LU_THREADS) void k_st_solve(const float *__restrict__ S, const float *__restrict__ w, int n,
                                                         double *__restrict__ Aall, float *__restrict__ x, int *__restrict__ info)
{
    constexpr int NW = LU_THREADS / 64;
    __shared__ double rhs[2 * STEADY_MAX_H], lcol[2 * STEADY_MAX_H], rv[NW];
    __shared__ int ri[NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double *A = Aall + (size_t)b * n * n;
    const float *Sb = S + (size_t)b * n * n;
    for (int idx = tid; idx < n * n; idx += LU_THREADS) {
        const int i = idx / n, j = idx - i * n;
        A[idx] = (i == j ? 1.0 : 0.0) - (double)Sb[idx];
    }
    for (int i = tid; i < n; i += LU_THREADS) rhs[i] = (double)w[(size_t)b * n + i];
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < n; ++k) {
        // the pivot, by the rule of phx_dense_lu.inc; a non-finite entry wins and ends the solve
        double best = -1.0;
        int bi = k;
        for (int i = k + tid; i < n; i += LU_THREADS) {
            double v = fabs(A[(size_t)i * n + k]);
            if (!(v <= LU_DBL_MAX)) v = __builtin_huge_val();       // NaN or Inf
            if (v > best) {
                best = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (o > best || (o == best && oi < bi)) {
                best = o;
                bi = oi;
            }
        }
        if (lane == 0) {
            rv[wv] = best;
            ri[wv] = bi;
        }
        __syncthreads();
        double pmax = rv[0];
        int piv = ri[0];
#pragma unroll
        for (int q = 1; q < NW; ++q)
            if (rv[q] > pmax || (rv[q] == pmax && ri[q] < piv)) {
                pmax = rv[q];
                piv = ri[q];
            }
        if (!(pmax > 0.0) || pmax == __builtin_huge_val()) {      // uniform over the workgroup
            bad = k + 1;
            break;
        }
        if (piv != k) {
            for (int j = k + tid; j < n; j += LU_THREADS) {
                const double t = A[(size_t)k * n + j];
                A[(size_t)k * n + j] = A[(size_t)piv * n + j];
                A[(size_t)piv * n + j] = t;
            }
            if (tid == 0) {
                const double t = rhs[k];
                rhs[k] = rhs[piv];
                rhs[piv] = t;
            }
        }
        __syncthreads();                       // the rows are swapped; rv, ri are read
        const double pv = A[(size_t)k * n + k], rk = rhs[k];
        for (int i = k + 1 + tid; i < n; i += LU_THREADS) {
            const double l = A[(size_t)i * n + k] / pv;
            lcol[i] = l;
            rhs[i] -= l * rk;
        }
        __syncthreads();
        // the trailing block: a wave takes every sixteenth row, its lanes the columns; the pivot row's entry is read once
        for (int j = k + 1 + lane; j < n; j += 64) {
            const double pk = A[(size_t)k * n + j];
#pragma unroll 4
            for (int i = k + 1 + wv; i < n; i += NW) A[(size_t)i * n + j] -= lcol[i] * pk;
        }
        __syncthreads();
    }
    if (!bad) {
        for (int k = n - 1; k >= 0; --k) {
            if (tid == 0) rhs[k] = rhs[k] / A[(size_t)k * n + k];
            __syncthreads();
            const double xk = rhs[k];
            for (int i = tid; i < k; i += LU_THREADS) rhs[i] -= A[(size_t)i * n + k] * xk;
            __syncthreads();
        }
        int nf = 0;
        for (int i = tid; i < n; i += LU_THREADS) nf |= !finite_as_float(rhs[i]);
        if (__syncthreads_or(nf)) bad = -1;
    }
    for (int i = tid; i < n; i += LU_THREADS) x[(size_t)b * n + i] = bad ? 0.f : (float)rhs[i];
    if (tid == 0) info[b] = bad;
}

bool rj_params_ok(const phx_params *p, int B)
{
    return steady_shape_ok(p, B) && p->Ws && p->bs && p->Wp && p->bp && p->WaT;
}

// states of one launch: all of them while their partial blocks stay under RJ_WS_CAP, else a multiple of RJ_SB
int rj_chunk(int N, int H, int B)
{
    const rj_geom q = rj_geometry(N, H);
    const size_t per = (size_t)q.S * 2 * H * q.NC * sizeof(float);
    size_t fit = RJ_WS_CAP / per;
    fit = fit < RJ_SB ? RJ_SB : fit / RJ_SB * RJ_SB;
    return (size_t)B < fit ? B : (int)fit;
}

}  // namespace

extern "C" {

size_t phx_reduced_jacobian_workspace_bytes(int N, int H, int B)
{
    if (!steady_shape_ok(N, H, B)) return 0;
    const rj_geom q = rj_geometry(N, H);
    return (size_t)q.S * rj_chunk(N, H, B) * 2 * H * q.NC * sizeof(float);
}

int phx_reduced_jacobian(const phx_params *p, const float *y, const float *m, const float *r, int B, float *S, float *w,
                         float *hid, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rj_params_ok(p, B) || !y || !m || !S || !hid) return PHX_ERR_BAD_ARG;
    if ((r != nullptr) != (w != nullptr)) return PHX_ERR_BAD_ARG;       // w is written exactly where r is given
    const int N = p->N, H = p->H, H2 = 2 * H;
    if (!workspace || workspace_bytes < phx_reduced_jacobian_workspace_bytes(N, H, B)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const rj_geom q = rj_geometry(N, H);
    const int chunk = rj_chunk(N, H, B);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        rj_args a;
        a.y = y + (size_t)b0 * N;
        a.m = m + (size_t)b0 * N;
        a.r = r ? r + (size_t)b0 * N : nullptr;
        a.part = static_cast<float *>(workspace);
        a.B = nb;
        const int groups = (nb + RJ_SB - 1) / RJ_SB;
        hipLaunchKernelGGL(k_rj, dim3((unsigned)(groups * q.S * q.nblk)), dim3(ST_THREADS), 0, st, p->Ws, p->Wp, p->WaT, N, H, a);
        if (!launched()) return PHX_ERR_LAUNCH;
        hipLaunchKernelGGL(k_rj_finish, dim3((unsigned)(nb * H2)), dim3(128), 0, st, a.part, p->bs, p->bp, H, q.NC, q.S, nb,
                           S + (size_t)b0 * H2 * H2, w ? w + (size_t)b0 * H2 : nullptr, hid + (size_t)b0 * H2);
        if (!launched()) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}

int phx_steady_residual(const phx_params *p, const float *y, int B, float *hid, float *r, void *stream)
{
    if (!rj_params_ok(p, B) || !y || !hid || !r || B > 65535) return PHX_ERR_BAD_ARG;
    const int N = p->N, H = p->H, H2 = 2 * H;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_st_hidden, dim3((unsigned)((H2 + ST_ROWS - 1) / ST_ROWS), (unsigned)B), dim3(ST_THREADS), 0, st, p->Ws,
                       p->bs, p->Wp, p->bp, N, H, y, hid);
    if (!launched()) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL(k_st_wa, dim3((unsigned)((N + ST_THREADS - 1) / ST_THREADS), (unsigned)B), dim3(ST_THREADS), 0, st, p->WaT,
                       N, H2, hid, y, (const float *)nullptr, (const float *)nullptr, 0, r);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

int phx_steady_update(const phx_params *p, const float *y, const float *m, const float *r, const float *x, int B, float *out,
                      void *stream)
{
    if (!steady_shape_ok(p, B) || !p->WaT || !y || !m || !r || !x || !out || B > 65535) return PHX_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_st_wa, dim3((unsigned)((p->N + ST_THREADS - 1) / ST_THREADS), (unsigned)B), dim3(ST_THREADS), 0,
                       (hipStream_t)stream, p->WaT, p->N, 2 * p->H, x, y, m, r, 1, out);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

size_t phx_steady_solve_workspace_bytes(int H, int B)
{
    if (!steady_shape_ok(/* N */ 1, H, B)) return 0;
    return (size_t)B * 4 * H * H * sizeof(double);
}

int phx_steady_solve(const float *S, const float *w, int H, int B, float *x, int *info, void *workspace, size_t workspace_bytes,
                     void *stream)
{
    if (!S || !w || !x || !info || !steady_shape_ok(/* N */ 1, H, B)) return PHX_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < phx_steady_solve_workspace_bytes(H, B)) return PHX_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_st_solve, dim3((unsigned)B), dim3(LU_THREADS), 0, (hipStream_t)stream, S, w, 2 * H,
                       static_cast<double *>(workspace), x, info);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // extern "C"
