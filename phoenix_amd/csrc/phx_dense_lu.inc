// phx_dense_lu.inc -- the steps of a dense LU with partial pivoting in double, one workgroup of THREADS threads per matrix:
// k_sr_inverse (phx_steady_resp.hip, [A | I]) runs its k loop over them.  k_st_solve (phx_steady.hip, A x = w) follows the
// same rule with the steps written out beside its right-hand side in LDS, because it measured slower through these
// calls: a change of the pivot rule is made in both places.  The range constants and finite_as_float are shared.  A is
// row-major with a row stride of ld doubles, in global memory.  Included inside an anonymous namespace after
// <hip/hip_runtime.h>.  (k_hill_steady, phx_hillss.hip, keeps an LU of its own: it lives in LDS, one wave finds the pivot,
// and a failed pivot means something else there.)

constexpr double LU_DBL_MAX = 1.7976931348623157e308;
constexpr float LU_FLT_MAX = 3.4028234663852886e38f;

// what a result stored as float must pass: an entry beyond the float range counts as not finite
__device__ __forceinline__ bool finite_as_float(float v) { return fabsf(v) <= LU_FLT_MAX; }
__device__ __forceinline__ bool finite_as_float(double v) { return finite_as_float((float)v); }

// The pivot row of column k: the largest |A[i][k]| over k <= i < n, the smallest i among equals; NaN or Inf counts as
// +huge, so a non-finite entry wins.  False where the column has no finite non-zero pivot (uniform over the workgroup).
// rv, ri: THREADS / 64 entries of LDS.  One barrier inside; the caller's next barrier comes before rv, ri are written again.
template <int THREADS>
__device__ __forceinline__ bool pivot(const double *A, int ld, int n, int k, double *rv, int *ri, int &piv)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double best = -1.0;
    int bi = k;
    for (int i = k + tid; i < n; i += THREADS) {
        double v = fabs(A[(size_t)i * ld + k]);
        if (!(v <= LU_DBL_MAX)) v = __builtin_huge_val();
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
    piv = ri[0];
#pragma unroll
    for (int q = 1; q < THREADS / 64; ++q)
        if (rv[q] > pmax || (rv[q] == pmax && ri[q] < piv)) {
            pmax = rv[q];
            piv = ri[q];
        }
    return pmax > 0.0 && pmax != __builtin_huge_val();
}

// rows k and piv change places in columns k .. ncols - 1
template <int THREADS>
__device__ __forceinline__ void swap_rows(double *A, int ld, int k, int piv, int ncols)
{
    for (int j = k + threadIdx.x; j < ncols; j += THREADS) {
        const double t = A[(size_t)k * ld + j];
        A[(size_t)k * ld + j] = A[(size_t)piv * ld + j];
        A[(size_t)piv * ld + j] = t;
    }
}

// A[i][j] -= lcol[i] A[k][j] for r0 <= i < r1, c0 <= j < ncols: a wave takes every (THREADS / 64)-th row, its lanes the
// columns; the entry of row k is read once.  Every entry is updated by one thread.
template <int THREADS>
__device__ __forceinline__ void eliminate(double *A, int ld, int k, int r0, int r1, int c0, int ncols, const double *lcol)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = c0 + lane; j < ncols; j += 64) {
        const double pk = A[(size_t)k * ld + j];
#pragma unroll 4
        for (int i = r0 + wv; i < r1; i += THREADS / 64) A[(size_t)i * ld + j] -= lcol[i] * pk;
    }
}
