// phx_effects_tile.inc -- the 64 x 64 tile engine shared by phx_effects.hip (which stores the tile) and its epilogue units
// phx_edges.hip, phx_netscore.hip, phx_neighbors.hip (which select from it) and phx_apply.hip (which sums it): the LDS image, the K loops and
// efx_tile<MODE>, which leaves one finished tile of the regulator -> target matrix in the MFMA accumulator layout, and
// behind them what the units share around the tile: the block-to-tile decoding, the parked tile, the tile pair of the
// oriented kernels, the argument checks and the <MODE, ORIENT> launch dispatch.  Included inside an anonymous namespace
// after <hip/hip_runtime.h>, <type_traits> and include/phoenix_hip.h; the layout and the chain order are described in
// phx_effects.hip.

constexpr int EFX_TILE = 64;       // regulators and targets of a workgroup
constexpr int EFX_LD = 144;        // floats of an LDS row: 64 regulator columns | 64 target columns | 16 padding
constexpr int EFX_THREADS = 256;   // four waves, 32 x 32 entries each
constexpr int EFX_MAX_H = 256;
constexpr int EFX_LDS_TAIL = 2 * EFX_MAX_H;   // two rows of p
constexpr int EFX_KC = 32;                  // hidden rows of an image of the effects mode (18 KiB)
constexpr int EFX_KU = 4;                   // K steps (of four hidden rows) whose operand reads are issued together
static_assert(EFX_MAX_H == EFX_THREADS, "thread t stages p[b, t]");

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// relu as torch computes it: a NaN multiplier stays NaN (fmaxf would turn it into 0)
__device__ __forceinline__ float efx_relu(float g) { return g > 0.f ? g : (g == g ? 0.f : g); }

// derivatives of SoftsignMod and LogShiftedSoftSignMod (odenet.py:21-35) in closed form, as phx_device.hpp: act_grad
__device__ __forceinline__ void efx_act_grad(float y, float &da, float &dl)
{
    const float s = y - 0.5f;
    const float d = 1.0f + fabsf(s);
    da = 1.0f / (d * d);
    dl = (s < 0.0f) ? 1.0f / d : 1.0f / ((1.0f + s) * (1.0f + 2.0f * s));
}

// image rows 0 .. rows - 1 = rows k0 .. of wi [H, N] (columns i0 .. i0 + 63) and of wj [H, N] (columns j0 .. j0 + 63), a
// quad of columns per thread and step (dword-aligned 16-byte loads, one ds_write_b128); zeros outside the matrices
__device__ __forceinline__ void efx_stage(float *img, const float *__restrict__ wi, const float *__restrict__ wj, int i0, int j0,
                                          int N, int H, int k0, int rows)
{
    for (int idx = threadIdx.x; idx < rows * (2 * EFX_TILE / 4); idx += EFX_THREADS) {
        const int kr = idx >> 5, c = (idx & 31) * 4, k = k0 + kr;
        const int col = c < EFX_TILE ? i0 + c : j0 + c - EFX_TILE;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < H && col < N) {
            const float *src = (c < EFX_TILE ? wi : wj) + (size_t)k * N + col;
            if (col + 3 < N) {
                __builtin_memcpy(&v, src, sizeof(f4));
            } else {
                v[0] = src[0];
                if (col + 1 < N) v[1] = src[1];
                if (col + 2 < N) v[2] = src[2];
            }
        }
        *reinterpret_cast<f4 *>(img + kr * EFX_LD + c) = v;
    }
}

// acc[ti][tj] += sum over the image's rows of  B(regulator tile ti) * A(target tile tj);  SCALE: row k of the regulator
// panel is multiplied by pp[k] first (pa, pb, pp already point at this lane's k = lane >> 4)
// one step: four k (this lane holds k = lane >> 4 of them)
template <bool SCALE>
__device__ __forceinline__ void efx_kstep(float a0, float a1, float b0, float b1, float s, f4 (&acc)[2][2])
{
    if (SCALE) {
        b0 *= s;
        b1 *= s;
    }
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a1, b0, acc[0][1]);
    acc[1][0] = mfma4(a0, b1, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
}

template <bool SCALE>
__device__ __forceinline__ void efx_kloop(const float *pa, const float *pb, const float *pp, int nk, f4 (&acc)[2][2])
{
    // four steps at a time: their 16 operand reads are issued together and the 16 MFMAs wait for them one step after the
    // other, so the LDS latency is paid once per group even with one wave per SIMD (k ascends as in the plain loop)
    int kk = 0;
    for (; kk + EFX_KU <= nk; kk += EFX_KU) {
        float a0[EFX_KU], a1[EFX_KU], b0[EFX_KU], b1[EFX_KU], s[EFX_KU];
#pragma unroll
        for (int u = 0; u < EFX_KU; ++u) {
            a0[u] = pa[4 * u * EFX_LD];
            a1[u] = pa[4 * u * EFX_LD + 16];
            b0[u] = pb[4 * u * EFX_LD];
            b1[u] = pb[4 * u * EFX_LD + 16];
            s[u] = SCALE ? pp[4 * u] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < EFX_KU; ++u) efx_kstep<SCALE>(a0[u], a1[u], b0[u], b1[u], s[u], acc);
        pa += 4 * EFX_KU * EFX_LD;
        pb += 4 * EFX_KU * EFX_LD;
        if (SCALE) pp += 4 * EFX_KU;
    }
    for (; kk < nk; ++kk) {
        efx_kstep<SCALE>(pa[0], pa[16], pb[0], pb[16], SCALE ? pp[0] : 1.f, acc);
        pa += 4 * EFX_LD;
        pb += 4 * EFX_LD;
        if (SCALE) pp += 4;
    }
}

// The finished tile (regulators i0 .. i0 + 63, targets j0 .. j0 + 63) of the matrix of MODE, in the accumulator layout:
// with lc = lane & 15, lq = lane >> 4 and this wave's corner (iw, jw) = (32 (wave & 1), 32 (wave >> 1)),
//     v[ti][tj][r] = entry (i0 + iw + 16 ti + lc,  j0 + jw + 16 tj + 4 lq + r)
// (the mean over the states first, then the scale by relu(g_j); entries outside the matrix hold unspecified finite-or-not
// values and must be masked by the caller).  Every thread of the workgroup calls it; the image in `lds`
// (effects_lds_bytes) is free again after the caller's next __syncthreads().
template <int MODE>
__device__ __forceinline__ void efx_tile(float *lds, const float *__restrict__ Ws, const float *__restrict__ Wp,
                                         const float *__restrict__ WaT, const float *__restrict__ g,
                                         const float *__restrict__ y, const float *__restrict__ ph, int N, int H, int B,
                                         int i0, int j0, f4 (&v)[2][2])
{
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hp = (H + 3) & ~3, nk = Hp >> 2;
    float *img = lds, *phs = lds + Hp * EFX_LD;                  // phs [2][EFX_MAX_H]
    const int iw = (wv & 1) * 32, jw = (wv >> 1) * 32;           // this wave's corner inside the tile
    const float *pb = img + lq * EFX_LD + iw + lc;               // regulator panel, B operand
    const float *pa = img + lq * EFX_LD + EFX_TILE + jw + lc;    // target panel, A operand
    const f4 zero = {0.f, 0.f, 0.f, 0.f};

    f4 S[2][2] = {{zero, zero}, {zero, zero}};
    f4 acc[2][2] = {{zero, zero}, {zero, zero}};
    if (MODE == PHX_EFFECTS) {
        // one accumulator over [Ws ; WaT[0:H]] and then [Wp ; WaT[H:2H]], EFX_KC rows at a time: the image is small, so
        // several workgroups share a CU (eight by LDS and the wave limit: an estimate) and the staging of one can run
        // under the MFMAs of the others
        for (int half = 0; half < 2; ++half) {
            const float *wi = half ? Wp : Ws, *wj = WaT + (size_t)half * H * N;
            for (int k0 = 0; k0 < Hp; k0 += EFX_KC) {
                const int rows = min(EFX_KC, Hp - k0);
                __syncthreads();                                 // every wave is done with the previous rows
                efx_stage(img, wi, wj, i0, j0, N, H, k0, rows);
                __syncthreads();
                efx_kloop<false>(pa, pb, nullptr, rows >> 2, acc);
            }
        }
    } else {
        efx_stage(img, Ws, WaT, i0, j0, N, H, 0, Hp);
        __syncthreads();
        efx_kloop<false>(pa, pb, nullptr, nk, S);
        __syncthreads();                                         // every wave is done with the first image
        efx_stage(img, Wp, WaT + (size_t)H * N, i0, j0, N, H, 0, Hp);
        phs[tid] = tid < H ? ph[tid] : 0.f;
        __syncthreads();
        int ig[2];                                               // this lane's two regulators
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) ig[ti] = i0 + iw + 16 * ti + lc;
        float yn[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) yn[ti] = ig[ti] < N ? y[ig[ti]] : 0.5f;
        for (int b = 0; b < B; ++b) {
            // what state b + 1 needs from memory is asked for now and used after this state's products
            const float pn = (b + 1 < B && tid < H) ? ph[(size_t)(b + 1) * H + tid] : 0.f;
            float yv[2];
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                yv[ti] = yn[ti];
                if (b + 1 < B && ig[ti] < N) yn[ti] = y[(size_t)(b + 1) * N + ig[ti]];
            }
            f4 Q[2][2] = {{zero, zero}, {zero, zero}};
            efx_kloop<true>(pa, pb, phs + (b & 1) * EFX_MAX_H + lq, nk, Q);
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                float da, dl;
                efx_act_grad(yv[ti], da, dl);
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const int jb = j0 + jw + 16 * tj + 4 * lq;   // first of this lane's four targets
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float e = fmaf(dl, Q[ti][tj][r], da * S[ti][tj][r]);
                        if (ig[ti] == jb + r) e -= 1.0f;
                        acc[ti][tj][r] += MODE == PHX_JAC_MEAN_ABS ? fabsf(e) : e;
                    }
                }
            }
            phs[((b + 1) & 1) * EFX_MAX_H + tid] = pn;
            __syncthreads();                                     // p of state b is read, p of state b + 1 is written
        }
    }

    const float fB = (float)B;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jb = j0 + jw + 16 * tj + 4 * lq;
        f4 rj;
#pragma unroll
        for (int r = 0; r < 4; ++r) rj[r] = jb + r < N ? efx_relu(g[jb + r]) : 0.f;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            f4 e = acc[ti][tj];
            if (MODE != PHX_EFFECTS) e = e / fB;                 // the mean first: a sum of B ones leaves as exactly 1
            v[ti][tj] = e * rj;
        }
    }
}

inline bool effects_shape_ok(int N, int H) { return N >= 2 && H >= 1 && H <= EFX_MAX_H; }

inline size_t effects_lds_bytes(int H, int mode)
{
    const int Hp = (H + 3) & ~3;
    if (mode == PHX_EFFECTS) return (size_t)(Hp < EFX_KC ? Hp : EFX_KC) * EFX_LD * sizeof(float);
    return ((size_t)Hp * EFX_LD + EFX_LDS_TAIL) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------------------------
// What the epilogue kernels (k_edges, k_gather, k_rank, k_neighbors) share around the tile.  Device side first.
constexpr int EFX_TLD = 68;                          // floats of a row of a parked tile: a lane's four rows lie 16 banks apart
constexpr int EFX_TBUF = EFX_TILE * EFX_TLD;         // 4352 floats
constexpr unsigned EFX_INF = 0x7f800000u;            // magnitude bits m < EFX_INF: finite;  m <= EFX_INF: not a NaN

// The tile (I, J) of workgroup blockIdx.x on the T x T tile grid; with `orient` the unordered pair I <= J of the
// T (T + 1) / 2 workgroups of efx_pair_grid
__device__ __forceinline__ void efx_tile_of_block(bool orient, int T, int &I, int &J)
{
    if (orient) {
        // blockIdx.x = J (J + 1) / 2 + I with I <= J: the root by float, then made exact
        const int p = blockIdx.x;
        J = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while ((J + 1) * (J + 2) / 2 <= p) ++J;
        while (J * (J + 1) / 2 > p) --J;
        I = p - J * (J + 1) / 2;
    } else {
        I = blockIdx.x / T;
        J = blockIdx.x - I * T;
    }
}

// parks a tile of the accumulator layout in LDS, ta[il * EFX_TLD + jl] = entry (i0 + il, j0 + jl), as four 16-byte stores,
// and with `both` a second tile vb in tb the same way, quad by quad beside the first.  (row, col) = (iw + lc, jw + 4 lq),
// this lane's first entry in the tile: the caller has them from its kernel's entry
__device__ __forceinline__ void efx_park(float *ta, const f4 (&va)[2][2], float *tb, const f4 (&vb)[2][2], bool both, int row,
                                         int col)
{
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            *reinterpret_cast<f4 *>(ta + (row + 16 * ti) * EFX_TLD + col + 16 * tj) = va[ti][tj];
            if (both) *reinterpret_cast<f4 *>(tb + (row + 16 * ti) * EFX_TLD + col + 16 * tj) = vb[ti][tj];
        }
}

// Leaves va = tile (I, J) and vp[ti][tj][r] = M[j, i] for the entry (i, j) of va[ti][tj][r]: forms tile (J, I) in the same
// image (a diagonal tile is its own partner), parks it over the dead image (EFX_TBUF floats at `lds`) and reads it back
// transposed, so that one lane holds both directions of a gene pair.  (row, col) as for efx_park.  between() runs after
// the store of the partner tile and before the barrier in front of the transposed read: the place for a caller's own LDS
// setup outside those EFX_TBUF floats.  Every thread of the workgroup calls it; tile (I, J) alone costs no barrier, the
// partner three (two when I == J).
template <int MODE, class Between>
__device__ __forceinline__ void efx_tile_pair(float *lds, const float *__restrict__ Ws, const float *__restrict__ Wp,
                                              const float *__restrict__ WaT, const float *__restrict__ g,
                                              const float *__restrict__ y, const float *__restrict__ ph, int N, int H, int B,
                                              int I, int J, int row, int col, f4 (&va)[2][2], f4 (&vp)[2][2], Between between)
{
    const int i0 = I * EFX_TILE, j0 = J * EFX_TILE;
    efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, i0, j0, va);
    f4 vb[2][2];                   // tile (J, I)
    if (I != J) {
        __syncthreads();           // every wave is done with the image of tile (I, J)
        efx_tile<MODE>(lds, Ws, Wp, WaT, g, y, ph, N, H, B, j0, i0, vb);
    } else {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) vb[ti][tj] = va[ti][tj];
    }
    __syncthreads();               // the image is dead: the transposed tile takes its place
    efx_park(lds, vb, lds, vb, false, row, col);
    between();
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) vp[ti][tj][r] = lds[(col + 16 * tj + r) * EFX_TLD + row + 16 * ti];
}

// Host side: the argument checks and the launch dispatch of the four entry points.
inline bool efx_mode_ok(int mode) { return mode == PHX_EFFECTS || mode == PHX_JAC_MEAN || mode == PHX_JAC_MEAN_ABS; }

// the shapes of the kernels whose keys hold i N + j in 32 bits (or a gene index in 16)
inline bool efx_pair_shape_ok(int N, int H) { return effects_shape_ok(N, H) && N <= 65535; }

// p and its four pointers, the shape (effects_shape_ok: a caller with keys adds efx_pair_shape_ok), the mode, the states of
// the Jacobian modes and the flag bits
inline bool efx_args_ok(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int allowed_flags)
{
    if (!p || !p->Ws || !p->Wp || !p->WaT || !p->g || !effects_shape_ok(p->N, p->H)) return false;
    if (!efx_mode_ok(mode)) return false;
    if (mode != PHX_EFFECTS && (!y || !ph || B < 1)) return false;
    return !(flags & ~allowed_flags);
}

// workgroups of a kernel that decodes its tile with efx_tile_of_block
inline int efx_pair_grid(int N, bool orient)
{
    const int T = (N + EFX_TILE - 1) / EFX_TILE;
    return orient ? T * (T + 1) / 2 : T * T;
}

// launch(MODE, ORIENT, y, ph, B) with the (checked) mode and the orientation as std::integral_constant arguments, so that a
// generic lambda picks its kernel instantiation from their types; PHX_EFFECTS has no states: (nullptr, nullptr, 1)
template <class Launch>
int efx_dispatch(int mode, bool orient, const float *y, const float *ph, int B, Launch &&launch)
{
    if (mode == PHX_EFFECTS) {
        y = ph = nullptr;
        B = 1;
    }
    const auto oriented = [&](auto MODE) {
        return orient ? launch(MODE, std::true_type(), y, ph, B) : launch(MODE, std::false_type(), y, ph, B);
    };
    switch (mode) {
    case PHX_EFFECTS: return oriented(std::integral_constant<int, PHX_EFFECTS>());
    case PHX_JAC_MEAN: return oriented(std::integral_constant<int, PHX_JAC_MEAN>());
    default: return oriented(std::integral_constant<int, PHX_JAC_MEAN_ABS>());
    }
}
