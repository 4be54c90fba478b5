// phx_screen_score.inc -- the front end shared by the scoring passes of the perturbation screens: phx_influence.hip,
// phx_knockout.hip and phx_epistasis.hip.  Each pass reads NS streams of the solver's output blocks ([T, calls * B, N];
// the tau = 0 slab, the initial states, is never touched), forms NQ terms per row and gene, and leaves their sums over the
// outputs tau = 1 .. T-1 and rows b < B in NQ matrices [K, N], and from the |.| sums one or two scores per screen row,
// in two plain launches:
//
//   the sum kernel    (scr_walk) grid (ceil(N / 256), K), W waves per workgroup.  A lane owns four adjacent gene columns
//                     (one 16-byte load per stream, row and lane, 1 KiB per wave instruction; gfx950 global loads need
//                     dword alignment only, so rows of an N that is no multiple of 4 are read the same way) and adds its
//                     terms in row order.  The (T-1) B rows are dealt round-robin to the W waves; the W partial sums meet
//                     in LDS and wave 0 adds them in wave order.  W depends on the shape alone, so the order of every sum
//                     is fixed: no atomics, two runs agree bit for bit.
//   the score kernel  (scr_score) one workgroup per screen row: thread t adds the |.| sums of columns t, t + 256, ... in
//                     order, skipping the held columns BY INDEX (never by subtracting them from a total), then a fixed
//                     LDS tree; it also scales the sums to means in place where the caller wants the matrices.  The scores
//                     are formed from the unscaled sums either way.
//
// The ragged tail (N % 4 != 0): the lane that owns the last 1..3 columns loads the quad that ENDS at column N - 1 and
// stores only its own columns, so the hot loop has one shape for every lane and nothing is read past a row's end.  Rows
// too short for a quad (N < 4: one lane) take element loads.
//
// A pass supplies a term type: its NS input streams (`seek` and `load`; ScrStreams<NS> serves those with a pointer each) and
//     static constexpr int NQ;  static __device__ void add(f4 (&acc)[NQ], const f4 (&v)[NS]);
// (what a row contributes, accumulators in the order of the output matrices), a rule for W, and the number of held
// columns a score skips; its __global__ kernels only set up the streams and instantiate scr_walk / scr_score.
// Included inside an anonymous namespace after <hip/hip_runtime.h>, <climits>, <cstddef> and include/phoenix_hip.h.

constexpr int SCR_TILE = 256;            // gene columns of a workgroup: one quad per lane
constexpr int SCR_SCORE_THREADS = 256;
constexpr int SCR_IDX_PER_LAUNCH = 256;  // indices that travel as kernel arguments (1 KiB)

typedef float f4 __attribute__((ext_vector_type(4)));

// NI index lists (held genes, calls of a stream) of one launch's screen rows
template <int NI>
struct ScrIdx {
    static constexpr int ROWS = SCR_IDX_PER_LAUNCH / NI;
    int g[NI][ROWS];
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

// NS input streams of a term.  q[s]: row 0 of output time 0 of the call that stream s reads for this workgroup's screen
// row; slab[s]: the floats of one output time of that stream's block.
template <int NS_>
struct ScrStreams {
    static constexpr int NS = NS_;
    const float *q[NS];
    size_t slab[NS];
    // -> tau = 1, row 0, the lane's first loaded column
    __device__ __forceinline__ void seek(int cl)
    {
#pragma unroll
        for (int s = 0; s < NS; ++s) q[s] += slab[s] + cl;
    }
    // row `ro / N` of output time tau + 1 of every stream: quads, or (QUADS false) the lane's nc elements
    template <bool QUADS>
    __device__ __forceinline__ void load(f4 (&v)[NS], int tau, size_t ro, int nc) const
    {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float *p = q[s] + (size_t)tau * slab[s] + ro;
            v[s] = QUADS ? load4(p) : load_n(p, nc);
        }
    }
};

// rows r, r + nwv, ... < M of a wave's walk, UNROLL of them in flight: all their loads, then their terms in row order
template <class Term, bool QUADS, int UNROLL>
__device__ __forceinline__ void scr_rows(const Term &term, f4 (&acc)[Term::NQ], int &tau, int &b, int &r, int nwv, int M,
                                         int B, int N, int nc)
{
    for (; r + (UNROLL - 1) * nwv < M; r += UNROLL * nwv) {
        f4 v[UNROLL][Term::NS];
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) {
            term.template load<QUADS>(v[i], tau, (size_t)b * N, nc);
            advance(tau, b, nwv, B);
        }
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) Term::add(acc, v[i]);
    }
}

// The sum kernel's body.  out[a]: the [K, N] matrix of accumulator a, or null (not stored); `row`: the workgroup's row of
// them.
template <class Term, int UNROLL, int MAX_WAVES>
__device__ __forceinline__ void scr_walk(Term term, float *const (&out)[Term::NQ], int row, int T, int B, int N)
{
    constexpr int NQ = Term::NQ;
    __shared__ f4 part[NQ][MAX_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int c0 = blockIdx.x * SCR_TILE + lane * 4;      // first column this lane owns
    const int nc = min(4, N - c0);                        // columns it owns (<= 0: none)
    const bool quads = N >= 4;
    const int cl = (quads && nc > 0 && nc < 4) ? N - 4 : c0;   // first column it loads
    term.seek(cl);
    const int M = (T - 1) * B;
    f4 acc[NQ];
#pragma unroll
    for (int a = 0; a < NQ; ++a) acc[a] = f4{0.f, 0.f, 0.f, 0.f};
    if (nc > 0) {
        int tau = 0, b = 0, r = wv;
        advance(tau, b, wv, B);
        if (quads) {
            scr_rows<Term, true, UNROLL>(term, acc, tau, b, r, nwv, M, B, N, nc);
            scr_rows<Term, true, 1>(term, acc, tau, b, r, nwv, M, B, N, nc);      // the remainder
        } else {
            scr_rows<Term, false, 1>(term, acc, tau, b, r, nwv, M, B, N, nc);
        }
    }
#pragma unroll
    for (int a = 0; a < NQ; ++a) part[a][wv][lane] = acc[a];
    __syncthreads();
    if (wv != 0 || nc <= 0) return;
#pragma unroll
    for (int a = 0; a < NQ; ++a) acc[a] = part[a][0][lane];
    for (int w = 1; w < nwv; ++w) {
#pragma unroll
        for (int a = 0; a < NQ; ++a) acc[a] += part[a][w][lane];
    }
    // the loaded quad starts c0 - cl columns before the first owned one (0 when N < 4)
#pragma unroll
    for (int a = 0; a < NQ; ++a)
        if (out[a]) store_owned(out[a] + (size_t)row * N + cl, acc[a], nc, c0 - cl);
}

// The score kernel's body, for screen row k0 + blockIdx.x.  mat[0 .. NR-1]: the |.| sums, one score each:
// scores[i][row] = (sum of mat[i][row, n] over n not among the row's NH held genes) / (M (N - NH)).  mat[NR ..]: the signed
// sums beside them, NM matrices in all.  Bit i of `scale`: row `row` of mat[i] becomes means (sums / M) in place.
template <int NR, int NH, int NM>
__device__ __forceinline__ void scr_score(float *const (&mat)[NM], float *const (&scores)[NR], const ScrIdx<NH> &held,
                                          int k0, int N, int M, int scale)
{
    __shared__ float red[NR][SCR_SCORE_THREADS];
    const int tid = threadIdx.x;
    int gene[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) gene[h] = held.g[h][blockIdx.x];
    const size_t o = (size_t)(k0 + blockIdx.x) * N;
    const double dM = (double)M;
    float acc[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i] = 0.f;
    for (int n = tid; n < N; n += SCR_SCORE_THREADS) {
        bool keep = true;
#pragma unroll
        for (int h = 0; h < NH; ++h) keep = keep && n != gene[h];
        // the scored sums are all loaded before the first store: the matrices are distinct, which the compiler cannot know
        float v[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = mat[i][o + n];
#pragma unroll
        for (int i = 0; i < NR; ++i)
            if (keep) acc[i] += v[i];
#pragma unroll
        for (int i = 0; i < NR; ++i)
            if (scale >> i & 1) mat[i][o + n] = (float)((double)v[i] / dM);
#pragma unroll
        for (int i = NR; i < NM; ++i)
            if (scale >> i & 1) mat[i][o + n] = (float)((double)mat[i][o + n] / dM);
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) red[i][tid] = acc[i];
    for (int h = SCR_SCORE_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int i = 0; i < NR; ++i) red[i][tid] += red[i][tid + h];
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i)
            scores[i][k0 + blockIdx.x] = (float)((double)red[i][0] / (dM * (double)(N - NH)));
    }
}

// ---- host side ----

// a [K, N] float matrix in a workspace
size_t scr_matrix_bytes(int K, int N) { return ((size_t)K * N * sizeof(float) + 255) / 256 * 256; }

// K screen rows of B solver rows each: the grid's y extent and the 32-bit row counts of the kernels
bool scr_shape_ok(int T, int K, int B, int N, int min_n)
{
    return T >= 2 && K >= 1 && B >= 1 && N >= min_n && K <= 65535 && (long long)(T - 1) * B <= INT_MAX &&
           (long long)K * B <= INT_MAX;
}

bool scr_in_range(const int *genes, int n, int N)
{
    for (int i = 0; i < n; ++i)
        if (genes[i] < 0 || genes[i] >= N) return false;
    return true;
}

// waves per workgroup where a launch's workgroups depend on K: rows are split over more waves until the launch has
// `target` of them (a function of the shape alone: the summation order must not depend on the device)
int scr_waves_filling(int T, int K, int B, int N, int max_waves, int target)
{
    const long long wgs = (long long)((N + SCR_TILE - 1) / SCR_TILE) * K, M = (long long)(T - 1) * B;
    int W = 1;
    while (W < max_waves && wgs * W < target && 2 * W <= M) W *= 2;
    return W;
}

dim3 scr_sum_grid(int N, int rows) { return dim3((N + SCR_TILE - 1) / SCR_TILE, rows); }

// list l, entry i = value(l, k0 + i) for the nk screen rows of a launch; zeros behind them
template <int NI, class F>
ScrIdx<NI> scr_pack(int k0, int nk, F value)
{
    ScrIdx<NI> x = {};
    for (int l = 0; l < NI; ++l)
        for (int i = 0; i < nk; ++i) x.g[l][i] = value(l, k0 + i);
    return x;
}

bool scr_launched() { return hipGetLastError() == hipSuccess; }

// launch(k0, nk) for the K screen rows in chunks of what ScrIdx<NI> holds; it returns scr_launched() of what it launched
template <int NI, class F>
int scr_for_chunks(int K, F launch)
{
    for (int k0 = 0; k0 < K; k0 += ScrIdx<NI>::ROWS) {
        const int nk = K - k0 < ScrIdx<NI>::ROWS ? K - k0 : ScrIdx<NI>::ROWS;
        if (!launch(k0, nk)) return PHX_ERR_LAUNCH;
    }
    return PHX_OK;
}
