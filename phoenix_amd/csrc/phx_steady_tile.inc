// phx_steady_tile.inc -- what the 64 x 64 tile kernels of the steady-state family share: k_rj (phx_steady.hip), k_sa_project
// and k_sa_pgrads (phx_steady_adj.hip), k_sr_response (phx_steady_resp.hip).  Each is a workgroup of 256 threads, four waves
// of 32 x 32 outputs on v_mfma_f32_16x16x4_f32, that walks its contraction TILE_KC steps at a time through panels in LDS.
// What a kernel stages, and from where, and how it stores its accumulators stays in the kernel; here are the types, the
// lane geometry, the K loop over a staged chunk, the ordered sum of the segments' partial blocks, and behind them the
// family's host-side checks.  Included inside an anonymous namespace after <hip/hip_runtime.h> and include/phoenix_hip.h.

constexpr int TILE = 64;                  // rows and columns of a workgroup's block
constexpr int TILE_KC = 32;               // contraction steps of a staged chunk
constexpr int TILE_LD = TILE_KC + 2;      // floats of a row of a row-major panel (64 rows of one chunk): the ds_read_b32 of
                                          // an MFMA operand, lane (lc, lq) at row lc, float lq, meets 32 distinct banks per
                                          // half wave
constexpr int TILE_LDK = TILE + 16;       // floats of a row of a K-major panel (one step of 64 columns): lane (lc, lq) at
                                          // float 80 lq + lc, 32 distinct banks per half wave
constexpr int ST_THREADS = 256;           // threads of every workgroup of the family but the LU kernels and k_rj_finish
constexpr int STEADY_MAX_H = 256;         // the H limit of include/phoenix_hip.h: LDS arrays of 2 H entries are sized by it

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the first nv floats at src, zeros behind them; src is not read where nv <= 0
__device__ __forceinline__ f4 ld4(const float *src, int nv)
{
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (nv >= 4) {
        __builtin_memcpy(&v, src, sizeof(f4));
    } else if (nv > 0) {
        v[0] = src[0];
        if (nv > 1) v[1] = src[1];
        if (nv > 2) v[2] = src[2];
    }
    return v;
}

// a quad into a row of TILE_LD floats: 8-byte aligned, not 16
__device__ __forceinline__ void st4(float *dst, f4 v)
{
    *reinterpret_cast<f2 *>(dst) = (f2){v[0], v[1]};
    *reinterpret_cast<f2 *>(dst + 2) = (f2){v[2], v[3]};
}

// a thread's place: lane (lc, lq) of wave wv, whose 32 x 32 outputs begin at (iw, jw) of the block.  Tile (ti, tj) of the
// wave holds rows 16 ti + 4 lq + r, r < 4, of column 16 tj + lc in acc[ti][tj][r].
struct tile_lane {
    int tid, lc, lq, wv, iw, jw;
};

__device__ __forceinline__ tile_lane tile_lanes()
{
    tile_lane L;
    L.tid = threadIdx.x;
    L.lc = L.tid & 15;
    L.lq = (L.tid & 63) >> 4;
    L.wv = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    L.iw = (L.wv & 1) * 32;
    L.jw = (L.wv >> 1) * 32;
    return L;
}

// how many of a wave's two 16-wide tiles from `first` on lie inside `extent` (uniform over the wave)
__device__ __forceinline__ int tiles_inside(int extent, int first) { return min(2, max(0, (extent - first + 15) / 16)); }

// the chunks [t_begin, t_end) of segment seg where T chunks are cut into S segments
__device__ __forceinline__ void seg_range(int seg, int T, int S, int &t_begin, int &t_end)
{
    t_begin = (int)((long long)seg * T / S);
    t_end = (int)((long long)(seg + 1) * T / S);
}

// staging of two row-major panels, a quad per thread and step: quad idx is floats c4 .. c4 + 3 of row rr of the panel
struct tile_quad {
    int panel, rr, c4;
};

__device__ __forceinline__ tile_quad tile_quad_at(int idx) { return {idx >> 9, (idx >> 3) & 63, (idx & 7) * 4}; }

// acc[ti][tj] += A(16 rows of tile ti) x B(16 columns of tile tj) over one chunk, K ascending.  Element (row, k) of a panel
// lies at row * RS + k * KS; pa, pb0, pb1 point at the lane's (row lc, step lq) of the wave's first tile; tile ti of A pairs
// with the panel pb<ti>.  ni, nj: the wave's tiles inside the matrix (uniform over the wave).
template <int RS, int KS>
__device__ __forceinline__ void tile_kloop(const float *pa, const float *pb0, const float *pb1, int ni, int nj, f4 (&acc)[2][2])
{
#pragma unroll
    for (int kk = 0; kk < TILE_KC / 4; ++kk) {
        const int k = 4 * kk * KS;
        const float a0 = pa[k], b00 = pb0[k];
        acc[0][0] = mfma4(a0, b00, acc[0][0]);
        if (nj > 1) acc[0][1] = mfma4(a0, pb0[16 * RS + k], acc[0][1]);
        if (ni > 1) {
            const float a1 = pa[16 * RS + k];
            acc[1][0] = mfma4(a1, pb1[k], acc[1][0]);
            if (nj > 1) acc[1][1] = mfma4(a1, pb1[16 * RS + k], acc[1][1]);
        }
    }
}

// src[0] + src[stride] + ... + src[(S - 1) stride], added in that order: the segments' partial blocks in segment order.
// The order is the contract: with the MFMA chain inside a segment it fixes the bits of every sum of the family.
__device__ __forceinline__ float seg_sum(const float *src, int S, size_t stride)
{
    float s = src[0];
    for (int k = 1; k < S; ++k) s += src[k * stride];
    return s;
}

bool launched() { return hipGetLastError() == hipSuccess; }

// the shape every entry point of the family accepts (N genes, H hidden rows per branch, B states)
bool steady_shape_ok(int N, int H, int B) { return N >= 1 && H >= 1 && H <= STEADY_MAX_H && B >= 1; }
bool steady_shape_ok(const phx_params *p, int B) { return p && steady_shape_ok(p->N, p->H, B); }
