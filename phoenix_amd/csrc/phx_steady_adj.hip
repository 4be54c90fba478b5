// phx_steady_adj.hip -- the implicit adjoint of the steady-state solve (phoenix_amd.steady_states(differentiable=True),
// DESIGN.md section 8q).
//
// A steady state satisfies P r(y*) = 0, (I - P) y* = (I - P) y0 with r(y) = Wa h(y) - y and P = diag(m), m = 1 on the genes that
// move.  With gy = dL/dy*, by the implicit function theorem
//     b = WaT (m gy),   (I - S^T) q = b,   u = gy + C^T q,   lam = m u,   dL/dy0 = (1 - m) u
// with S = C P Wa, the matrix phx_reduced_jacobian writes, and the parameter gradients are contractions over the rows:
//     dWa[n, c] = sum_b lam[b, n] hid[b, c],   dWs[j, n] = sum_b q[b, j] a[b, n],   dWp[j, n] = sum_b q[b, H + j] v[b, j] l[b, n]
//     dbs[j] = sum_b q[b, j],   dbp[j] = sum_b q[b, H + j] v[b, j],   dg = 0.
//
//   k_sa_project  b [B, 2H]: a contraction over the genes, 64 rows x 64 columns per workgroup (four waves of 32 x 32), the
//                 gene axis cut into S = min(ceil(N / 32), 8) segments, a function of N alone.  32 genes of the 64 rows of
//                 m gy and of the 64 rows of WaT lie in LDS (the row-major panels of phx_steady_tile.inc, as in k_rj).
//                 k_sa_sum adds the segments' partial blocks in segment order.
//   k_sa_back     u = gy + C^T q of one row and 256 genes per workgroup, one thread per gene, j ascending: the transposed
//                 twin of k_st_wa.
//   k_sa_pgrads   the [4H] x (N + 1) block of the five products; the contraction runs over the rows.  Its columns are laid
//                 out in 16-wide tiles, each of one kind: ceil(H / 16) tiles of q (against a), ceil(H / 16) of q v (against
//                 l), ceil(2H / 16) of hid (against lam).  Gene N is a column of ones under a and l: its sums are the bias
//                 gradients.  A workgroup owns four column tiles x 64 genes and a segment of the rows; it walks the segment
//                 32 rows at a time.  The chunk's 64 columns and its (a, l, lam) of 64 genes lie in LDS row-major over the
//                 rows (the K-major panels of phx_steady_tile.inc; the staging stores are conflict-free); a and l are
//                 recomputed from y once per (row, gene) of the chunk.  v_mfma_f32_16x16x4_f32, rows ascending.
//                 The rows are cut into S = max(1, min(ceil(B / 32) / 2, ceil(512 / blocks))) segments, a function of
//                 (N, H, B) alone; k_sa_pg_rows / k_sa_pg_wa / k_sa_pg_small add the segments' partial blocks in segment
//                 order and write (or add to) the phx_grads buffers, every element once.
//   sum order     fixed by the shape alone; no atomics; two runs give the same bits.
// The lane geometry, the K loop and the ordered segment sum are those of phx_steady_tile.inc, shared with phx_steady.hip and
// phx_steady_resp.hip.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/phoenix_hip.h"
#include "phx_device.hpp"

namespace {

#include "phx_steady_tile.inc"

constexpr int PJ_SEGS = 8;            // most segments of the gene axis in k_sa_project
constexpr int PG_WGS = 512;           // workgroups that the row segments of k_sa_pgrads aim at

__host__ __device__ inline int pj_segments(int N)
{
    const int T = (N + TILE_KC - 1) / TILE_KC;
    return T < PJ_SEGS ? T : PJ_SEGS;
}

// part[seg][b][c] = sum over the genes of the segment of (m gy)[b, n] WaT[c, n]
__global__ __launch_bounds__(ST_THREADS) void k_sa_project(const float *__restrict__ WaT, int N, int H2, const float *__restrict__ m,
                                                           const float *__restrict__ gy, int B, float *__restrict__ part)
{
    __shared__ float pa_s[TILE * TILE_LD], pb_s[TILE * TILE_LD];
    const tile_lane L = tile_lanes();
    const int tid = L.tid;
    const int CB = (H2 + TILE - 1) / TILE, RB = (B + TILE - 1) / TILE, S = pj_segments(N), T = (N + TILE_KC - 1) / TILE_KC;
    const int cb = blockIdx.x % CB, rest = blockIdx.x / CB, rb = rest % RB, seg = rest / RB;
    const int row0 = rb * TILE, col0 = cb * TILE;
    int t_begin, t_end;
    seg_range(seg, T, S, t_begin, t_end);
    const int ni = tiles_inside(B, row0 + L.iw), nj = tiles_inside(H2, col0 + L.jw);
    const float *pa = pa_s + (L.iw + L.lc) * TILE_LD + L.lq, *pb = pb_s + (L.jw + L.lc) * TILE_LD + L.lq;

    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 acc[2][2] = {{zero, zero}, {zero, zero}};
    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TILE_KC;
        __syncthreads();                       // every wave is done with the previous chunk
#pragma unroll
        for (int u = 0; u < 2 * TILE * TILE_KC / 4 / ST_THREADS; ++u) {
            const tile_quad s = tile_quad_at(tid + u * ST_THREADS);
            const int n = n0 + s.c4, row = (s.panel ? col0 : row0) + s.rr;
            // nothing is read of a row outside the matrix or past a row's end, where `at` is out of range (ld4: nv <= 0)
            const int nv = row < (s.panel ? H2 : B) ? N - n : 0;
            const size_t at = (size_t)row * N + n;
            f4 v;
            if (s.panel == 0) {
                const f4 mv = ld4(m + at, nv), gv = ld4(gy + at, nv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = mv[e] != 0.f ? mv[e] * gv[e] : 0.f;     // a gene of weight 0 takes no part
            } else {
                v = ld4(WaT + at, nv);
            }
            st4((s.panel ? pb_s : pa_s) + s.rr * TILE_LD + s.c4, v);
        }
        __syncthreads();
        if (ni > 0 && nj > 0) tile_kloop<TILE_LD, 1>(pa, pb, pb, ni, nj, acc);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int c = col0 + L.jw + 16 * tj + L.lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + L.iw + 16 * ti + 4 * L.lq + r;
                if (row < B && c < H2) part[((size_t)seg * B + row) * H2 + c] = acc[ti][tj][r];
            }
        }
}

// out[i] = part[0][i] + part[1][i] + ... in that order
__global__ __launch_bounds__(ST_THREADS) void k_sa_sum(const float *__restrict__ part, int S, size_t total, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i < total) out[i] = seg_sum(part + i, S, total);
}

// u = gy + a' sum_j Ws[j, n] q[j] + l' sum_j Wp[j, n] v[j] q[H + j], j ascending;  lam = m u where m != 0, else 0;
// gy0 = u where m == 0, else 0
__global__ __launch_bounds__(ST_THREADS) void k_sa_back(const float *__restrict__ Ws, const float *__restrict__ Wp, int N, int H,
                                                        const float *__restrict__ y, const float *__restrict__ m,
                                                        const float *__restrict__ gy, const float *__restrict__ q,
                                                        const float *__restrict__ hid, float *__restrict__ lam, float *__restrict__ gy0)
{
    __shared__ float qs[2 * STEADY_MAX_H];
    const int b = blockIdx.y, n = blockIdx.x * ST_THREADS + threadIdx.x, H2 = 2 * H;
    for (int c = threadIdx.x; c < H2; c += ST_THREADS) {
        const float qv = q[(size_t)b * H2 + c];
        qs[c] = c < H ? qv : qv * hid[(size_t)b * H2 + c];
    }
    __syncthreads();
    if (n >= N) return;
    const size_t at = (size_t)b * N + n;
    float da, dl;
    phx::act_grad(y[at], da, dl);
    float zs = 0.f, zp = 0.f;
    for (int j = 0; j < H; ++j) {
        zs = fmaf(Ws[(size_t)j * N + n], qs[j], zs);
        zp = fmaf(Wp[(size_t)j * N + n], qs[H + j], zp);
    }
    const float u = fmaf(dl, zp, fmaf(da, zs, gy[at])), mv = m[at];
    lam[at] = mv != 0.f ? mv * u : 0.f;
    gy0[at] = mv != 0.f ? 0.f : u;
}

struct pg_geom {
    int T1, TT, CB, GB, T, S;
};

__host__ __device__ inline pg_geom pg_geometry(int N, int H, int B)
{
    pg_geom g;
    g.T1 = (H + 15) / 16;
    g.TT = 2 * g.T1 + (2 * H + 15) / 16;
    g.CB = (g.TT + 3) / 4;
    g.GB = (N + 1 + TILE - 1) / TILE;
    g.T = (B + TILE_KC - 1) / TILE_KC;
    const long long blocks = (long long)g.CB * g.GB;
    const int want = (int)((PG_WGS + blocks - 1) / blocks), half = g.T / 2;
    g.S = half < 1 ? 1 : (half < want ? half : want);
    return g;
}

// part[seg][r][n], r < 4H the rows of (dWs, dWp, dWaT), n <= N (n == N: the bias sums of the first 2H rows)
__global__ __launch_bounds__(ST_THREADS) void k_sa_pgrads(const float *__restrict__ y, const float *__restrict__ lam,
                                                          const float *__restrict__ q, const float *__restrict__ hid, int N, int H,
                                                          int B, float *__restrict__ part)
{
    __shared__ float xs[TILE_KC * TILE_LDK], gs[3 * TILE_KC * TILE_LDK];
    const tile_lane L = tile_lanes();
    const int tid = L.tid, H2 = 2 * H, NP = N + 1;
    const pg_geom g = pg_geometry(N, H, B);
    const int cb = blockIdx.x % g.CB, rest = blockIdx.x / g.CB, gb = rest % g.GB, seg = rest / g.GB;
    const int n0 = gb * TILE;
    int t_begin, t_end;
    seg_range(seg, g.T, g.S, t_begin, t_end);
    // the wave's column tiles: their kind (0: q against a, 1: q v against l, 2: hid against lam) and first output row
    const int ct0 = cb * 4 + (L.wv & 1) * 2;
    const int ni = min(2, max(0, g.TT - ct0)), nj = tiles_inside(NP, n0 + L.jw);
    int kind[2], orow[2], olim[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int ct = ct0 + ti;
        kind[ti] = ct < g.T1 ? 0 : (ct < 2 * g.T1 ? 1 : 2);
        const int c = 16 * (ct - kind[ti] * g.T1);                    // the tile's first column inside its kind
        orow[ti] = kind[ti] * H + c;
        olim[ti] = (kind[ti] == 2 ? H2 : H) - c;                      // columns of the tile inside the matrix
    }
    const float *pa = xs + L.lq * TILE_LDK + L.iw + L.lc;
    const float *pb0 = gs + (kind[0] * TILE_KC + L.lq) * TILE_LDK + L.jw + L.lc;
    const float *pb1 = gs + (kind[1] * TILE_KC + L.lq) * TILE_LDK + L.jw + L.lc;
    // what this thread stages: column rr of the workgroup's 64 and gene n0 + rr, rows (tid >> 6) + 4 u of the chunk
    const int rr = tid & 63, sct = cb * 4 + (rr >> 4);
    const int skind = sct < g.T1 ? 0 : (sct < 2 * g.T1 ? 1 : 2), sc = 16 * (sct - skind * g.T1) + (rr & 15);
    const bool sin = sct < g.TT && sc < (skind == 2 ? H2 : H);
    const int scol = skind == 1 ? H + sc : sc;                        // the column of q (kinds 0, 1) or hid (kind 2)
    const int sn = n0 + rr;

    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 acc[2][2] = {{zero, zero}, {zero, zero}};
    for (int t = t_begin; t < t_end; ++t) {
        const int bt0 = t * TILE_KC;
        __syncthreads();                       // every wave is done with the previous chunk
#pragma unroll
        for (int u = 0; u < TILE_KC / 4; ++u) {
            const int bb = (tid >> 6) + 4 * u, b = bt0 + bb;
            float xv = 0.f, av = 0.f, lv = 0.f, lm = 0.f;
            if (b < B) {
                if (sin) {
                    const size_t at = (size_t)b * H2 + scol;
                    xv = skind == 0 ? q[at] : (skind == 1 ? q[at] * hid[at] : hid[at]);
                }
                if (sn < N) {
                    const size_t at = (size_t)b * N + sn;
                    phx::act_pair(y[at], av, lv);
                    lm = lam[at];
                } else if (sn == N) {
                    av = 1.f;                  // the column of ones: the bias sums
                    lv = 1.f;
                }
            }
            xs[bb * TILE_LDK + rr] = xv;
            gs[(0 * TILE_KC + bb) * TILE_LDK + rr] = av;
            gs[(1 * TILE_KC + bb) * TILE_LDK + rr] = lv;
            gs[(2 * TILE_KC + bb) * TILE_LDK + rr] = lm;
        }
        __syncthreads();
        if (ni > 0 && nj > 0) tile_kloop<1, TILE_LDK>(pa, pb0, pb1, ni, nj, acc);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        if (ti >= ni) break;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int n = n0 + L.jw + 16 * tj + L.lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * L.lq + r;
                if (i < olim[ti] && n < NP) part[((size_t)seg * 2 * H2 + orow[ti] + i) * NP + n] = acc[ti][tj][r];
            }
        }
    }
}

// dst[r][n] (=, +=) the segments' sums of rows r0 + r of the partial blocks, r < rows, n < N
__global__ __launch_bounds__(ST_THREADS) void k_sa_pg_rows(const float *__restrict__ part, int S, int R4, int NP, int N, int r0,
                                                           float *__restrict__ dst, int overwrite)
{
    const int n = blockIdx.x * ST_THREADS + threadIdx.x, r = blockIdx.y;
    if (n >= N) return;
    const float s = seg_sum(part + (size_t)(r0 + r) * NP + n, S, (size_t)R4 * NP);
    float *o = dst + (size_t)r * N + n;
    *o = overwrite ? s : *o + s;
}

// Wa[n][c] (=, +=) the segments' sums of row 2H + c, through a 32 x 32 tile in LDS
__global__ __launch_bounds__(ST_THREADS) void k_sa_pg_wa(const float *__restrict__ part, int S, int R4, int NP, int N, int H2,
                                                         float *__restrict__ Wa, int overwrite)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, nb = blockIdx.x * 32, cbase = blockIdx.y * 32;
    const size_t stride = (size_t)R4 * NP;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = cbase + ty + 8 * u, n = nb + tx;
        tile[ty + 8 * u][tx] = c < H2 && n < N ? seg_sum(part + (size_t)(H2 + c) * NP + n, S, stride) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = nb + ty + 8 * u, c = cbase + tx;
        if (n < N && c < H2) {
            float *o = Wa + (size_t)n * H2 + c;
            *o = overwrite ? tile[tx][ty + 8 * u] : *o + tile[tx][ty + 8 * u];
        }
    }
}

// the bias gradients (column N of the first 2H rows), and g = 0 under overwrite
__global__ __launch_bounds__(ST_THREADS) void k_sa_pg_small(const float *__restrict__ part, int S, int R4, int NP, int N, int H,
                                                            float *__restrict__ dbs, float *__restrict__ dbp, float *__restrict__ dg,
                                                            int overwrite)
{
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    if (i < 2 * H) {
        const float s = seg_sum(part + (size_t)i * NP + N, S, (size_t)R4 * NP);
        float *o = i < H ? dbs + i : dbp + (i - H);
        *o = overwrite ? s : *o + s;
    }
    if (overwrite && i < N) dg[i] = 0.f;
}

}  // namespace

extern "C" {

size_t phx_steady_adjoint_project_workspace_bytes(int N, int H, int B)
{
    if (!steady_shape_ok(N, H, B)) return 0;
    return (size_t)pj_segments(N) * B * 2 * H * sizeof(float);
}

int phx_steady_adjoint_project(const phx_params *p, const float *m, const float *gy, int B, float *b, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!steady_shape_ok(p, B) || !p->WaT || !m || !gy || !b) return PHX_ERR_BAD_ARG;
    const int N = p->N, H2 = 2 * p->H;
    if (!workspace || workspace_bytes < phx_steady_adjoint_project_workspace_bytes(N, p->H, B)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int S = pj_segments(N), CB = (H2 + TILE - 1) / TILE, RB = (B + TILE - 1) / TILE;
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(k_sa_project, dim3((unsigned)((size_t)S * RB * CB)), dim3(ST_THREADS), 0, st, p->WaT, N, H2, m, gy, B, part);
    if (!launched()) return PHX_ERR_LAUNCH;
    const size_t total = (size_t)B * H2;
    hipLaunchKernelGGL(k_sa_sum, dim3((unsigned)((total + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0, st, part, S, total, b);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

int phx_steady_adjoint_back(const phx_params *p, const float *y, const float *m, const float *gy, const float *q, const float *hid,
                            int B, float *lam, float *gy0, void *stream)
{
    if (!steady_shape_ok(p, B) || !p->Ws || !p->Wp || !y || !m || !gy || !q || !hid || !lam || !gy0 || B > 65535)
        return PHX_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_sa_back, dim3((unsigned)((p->N + ST_THREADS - 1) / ST_THREADS), (unsigned)B), dim3(ST_THREADS), 0,
                       (hipStream_t)stream, p->Ws, p->Wp, p->N, p->H, y, m, gy, q, hid, lam, gy0);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

size_t phx_steady_param_grads_workspace_bytes(int N, int H, int B)
{
    if (!steady_shape_ok(N, H, B)) return 0;
    return (size_t)pg_geometry(N, H, B).S * 4 * H * ((size_t)N + 1) * sizeof(float);
}

int phx_steady_param_grads(const phx_params *p, const float *y, const float *lam, const float *q, const float *hid, int B,
                           const phx_grads *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!steady_shape_ok(p, B) || !y || !lam || !q || !hid || !grads) return PHX_ERR_BAD_ARG;
    if (!grads->Ws || !grads->bs || !grads->Wp || !grads->bp || !(grads->Wa || grads->WaT) || (grads->overwrite && !grads->g))
        return PHX_ERR_BAD_ARG;
    const int N = p->N, H = p->H, H2 = 2 * H, R4 = 4 * H, NP = N + 1;
    if (!workspace || workspace_bytes < phx_steady_param_grads_workspace_bytes(N, H, B)) return PHX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const pg_geom g = pg_geometry(N, H, B);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(k_sa_pgrads, dim3((unsigned)((size_t)g.S * g.GB * g.CB)), dim3(ST_THREADS), 0, st, y, lam, q, hid, N, H, B, part);
    if (!launched()) return PHX_ERR_LAUNCH;
    const unsigned nx = (unsigned)((N + ST_THREADS - 1) / ST_THREADS);
    const int ow = grads->overwrite != 0;
    hipLaunchKernelGGL(k_sa_pg_rows, dim3(nx, (unsigned)H), dim3(ST_THREADS), 0, st, part, g.S, R4, NP, N, 0, grads->Ws, ow);
    if (!launched()) return PHX_ERR_LAUNCH;
    hipLaunchKernelGGL(k_sa_pg_rows, dim3(nx, (unsigned)H), dim3(ST_THREADS), 0, st, part, g.S, R4, NP, N, H, grads->Wp, ow);
    if (!launched()) return PHX_ERR_LAUNCH;
    if (grads->Wa)
        hipLaunchKernelGGL(k_sa_pg_wa, dim3((unsigned)((N + 31) / 32), (unsigned)((H2 + 31) / 32)), dim3(ST_THREADS), 0, st, part, g.S,
                           R4, NP, N, H2, grads->Wa, ow);
    else
        hipLaunchKernelGGL(k_sa_pg_rows, dim3(nx, (unsigned)H2), dim3(ST_THREADS), 0, st, part, g.S, R4, NP, N, H2, grads->WaT, ow);
    if (!launched()) return PHX_ERR_LAUNCH;
    const int small = H2 > N ? H2 : N;
    hipLaunchKernelGGL(k_sa_pg_small, dim3((unsigned)((small + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0, st, part, g.S, R4,
                       NP, N, H, grads->bs, grads->bp, grads->g, ow);
    return launched() ? PHX_OK : PHX_ERR_LAUNCH;
}

}  // namespace extern "C"
