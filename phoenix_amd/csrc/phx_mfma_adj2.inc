// phx_mfma_adj2.inc -- backward pass of odeint_adjoint, second-generation kernel (replaces k1_solve_adj for hidden
// layers that stay LDS resident, H <= 128).  Same algorithm as phx_mfma_adj.inc / phx_adjoint.inc: the reverse-time
// augmented solve of adjoint.py:32-162 with the parameter gradient as a quadrature over the accepted steps.
//
// What is different (DESIGN.md "adjoint kernel, second generation"):
//   * WAVE PAIRS.  The augmented evaluation splits cleanly by state: everything that produces or consumes the
//     expression state y (activations a(y), l(y); u = Ws a, v = Wp l; j = Wa z; k_y) is one wave's work, everything
//     of the adjoint state a (q = a relu(g); dz = WaT q; a~ = Ws^T du, l~ = Wp^T dv; k_a) another's.  A 16-trajectory
//     tile is owned by a PAIR (y-wave, a-wave): 8 waves per workgroup = 2 per SIMD, each inside 256 registers,
//     equal MFMA counts (96 per gene block and evaluation each), no duplicated arithmetic.
//   * PAIRS ARE COROUTINES.  After the weights are staged there is no workgroup barrier: every wave keeps its own
//     copy of its tile's step controllers in LDS (deterministic => identical in both waves of a pair and in every
//     workgroup of the group), reduces the exchange rows it owns by itself, and meets its partner only through two
//     LDS words.  The pairs of a workgroup therefore drift apart, and the launch starts half of them late on purpose
//     (each SIMD hosts the y-wave of one pair and the a-wave of a pair of the other half): while one pair waits for
//     an exchange the other has the SIMD to itself, so exchange latency overlaps compute instead of adding to it.
//   * FUSED SWEEPS.  A stage's expansion products (P2': needs the reduced hidden rows) and the NEXT stage's
//     contraction products (P1': needs only this wave's own tiles) run in one sweep over the gene blocks; the new k
//     tile is consumed from registers; the tiles of block b+1 are requested before P1'(b) and P2'(b+1), which need no
//     tile data, so one memory round trip per block hides under 96 MFMAs.
//   * The quadrature reads its hidden-row operands from wave-private, already transposed copies (written once when
//     the rows are gathered), and derives the gene-multiplier term from k_y instead of storing a tile per stage.
//   * The dopri5 error estimate is accumulated while the last stage input is formed (the k tiles are in registers
//     then), so the last stage reads two tiles instead of twelve.
#ifndef PHX_QB
#define PHX_QB 1   // gene blocks whose gradient accumulators a wave keeps in registers (HT = 3)
#endif
namespace {

constexpr int NVEC_ADJ2 = 32;
constexpr int NP2_MAX = 4;             // wave pairs per workgroup: 4 (two waves per SIMD, 256 registers) or 2 (one, 512)
// private state vectors (tile-native scratch); side 0: expression state y, side 1: adjoint state a
__device__ __forceinline__ int vX0(int side) { return side; }
__device__ __forceinline__ int vE(int side) { return 2 + side; }                       // partial error estimate
__device__ __forceinline__ int vXS(int side, int slot) { return 4 + 7 * side + slot; }  // stage inputs
__device__ __forceinline__ int vK(int side, int slot) { return 18 + 7 * side + slot; }  // stage derivatives

// LDS behind the weight images: pair flags + timer block, then one controller block per wave
constexpr int ADJ2_WC_PER_TRAJ = 112;   // bytes: 4 doubles, 5 floats, 7 ints, 8 quadrature weights
constexpr int ADJ2_FLAG_BYTES = 512;
__host__ __device__ inline size_t adj2_ctl_bytes(int NP, int TPW) { return ADJ2_FLAG_BYTES + (size_t)2 * NP * ADJ2_WC_PER_TRAJ * 16 * TPW; }

struct WC2 {   // one wave's controllers: index i = (tile of the wave) * 16 + trajectory of the tile
    double *rk_t0, *rk_t1, *dt, *xfin;
    float *dtf, *dtp, *h0f, *sgn, *d1;
    int *done, *accept, *fin, *st, *nsteps, *nfe, *nsiv;
    float *wq;   // [n][8]
};
__device__ __forceinline__ WC2 carve_wc2(char *base, int n)
{
    WC2 c;
    double *dp = reinterpret_cast<double *>(base);
    c.rk_t0 = dp; c.rk_t1 = dp + n; c.dt = dp + 2 * n; c.xfin = dp + 3 * n;
    float *fp = reinterpret_cast<float *>(dp + 4 * n);
    c.dtf = fp; c.dtp = fp + n; c.h0f = fp + 2 * n; c.sgn = fp + 3 * n; c.d1 = fp + 4 * n;
    int *ip = reinterpret_cast<int *>(fp + 5 * n);
    c.done = ip; c.accept = ip + n; c.fin = ip + 2 * n; c.st = ip + 3 * n; c.nsteps = ip + 4 * n; c.nfe = ip + 5 * n;
    c.nsiv = ip + 6 * n;
    c.wq = reinterpret_cast<float *>(ip + 7 * n);
    return c;
}

struct Xg2 {
    unsigned int *abort_flag;
    bool aborted;
};

// wave-level: read NR rows (uniform base + 32-bit row offsets, in granules) until every lane of each carries `tag`
// (bounded spin, see phx_mfma_common.inc)
template <int NR>
__device__ __forceinline__ void wait_rows2(Xg2 &x, const u64 *base, const unsigned (&offs)[NR], int nvalid, unsigned int tag,
                                           unsigned lane, float (&out)[NR])
{
    unsigned int spins = 0;
    unsigned long long t_start = 0;
    for (;;) {
        u64 g[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) g[k] = (k < nvalid) ? ld_gran(base + (offs[k] + lane)) : ((u64)tag << 32);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NR; ++k) ok = ok && ((unsigned int)(g[k] >> 32) == tag);
#pragma unroll
        for (int k = 0; k < NR; ++k) out[k] = __uint_as_float((unsigned int)g[k]);
        if (__all(ok) || x.aborted) {
            asm volatile("" ::: "memory");   // nothing that follows may be moved ahead of the completed poll
            return;
        }
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0) {
            if (t_start == 0) t_start = wall_clock64();
            if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                wall_clock64() - t_start > 500000000ull) {
                __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.aborted = true;
                return;
            }
        }
    }
}

// wave-level: the same row of NR consecutive members (granule stride `stride`) in ONE batch of loads
template <int NR>
__device__ __forceinline__ void wait_members(Xg2 &x, const u64 *row0, unsigned stride, int nvalid, unsigned int tag,
                                             unsigned lane, float (&out)[NR])
{
    unsigned int spins = 0;
    unsigned long long t_start = 0;
    for (;;) {
        u64 g[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) g[k] = (k < nvalid) ? ld_gran(row0 + (size_t)k * stride + lane) : ((u64)tag << 32);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NR; ++k) ok = ok && ((unsigned int)(g[k] >> 32) == tag);
#pragma unroll
        for (int k = 0; k < NR; ++k) out[k] = __uint_as_float((unsigned int)g[k]);
        if (__all(ok) || x.aborted) {
            asm volatile("" ::: "memory");
            return;
        }
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0) {
            if (t_start == 0) t_start = wall_clock64();
            if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                wall_clock64() - t_start > 500000000ull) {
                __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.aborted = true;
                return;
            }
        }
    }
}

// wave-level: NRW rows (granule stride `rstride` between them), each from NM consecutive members (granule stride
// `mstride`), in ONE batch of loads: out[r][m]; rows >= nrows / members >= nmem are not read
template <int NRW, int NM>
__device__ __forceinline__ void wait_members_rows(Xg2 &x, const u64 *row0, unsigned rstride, unsigned mstride, int nrows,
                                                  int nmem, unsigned int tag, unsigned lane, float (&out)[NRW][NM])
{
    unsigned int spins = 0;
    unsigned long long t_start = 0;
    for (;;) {
        u64 g[NRW][NM];
#pragma unroll
        for (int r = 0; r < NRW; ++r)
#pragma unroll
            for (int k = 0; k < NM; ++k)
                g[r][k] = (r < nrows && k < nmem) ? ld_gran(row0 + (size_t)r * rstride + (size_t)k * mstride + lane)
                                                  : ((u64)tag << 32);
        bool ok = true;
#pragma unroll
        for (int r = 0; r < NRW; ++r)
#pragma unroll
            for (int k = 0; k < NM; ++k) ok = ok && ((unsigned int)(g[r][k] >> 32) == tag);
#pragma unroll
        for (int r = 0; r < NRW; ++r)
#pragma unroll
            for (int k = 0; k < NM; ++k) out[r][k] = __uint_as_float((unsigned int)g[r][k]);
        if (__all(ok) || x.aborted) {
            asm volatile("" ::: "memory");
            return;
        }
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0) {
            if (t_start == 0) t_start = wall_clock64();
            if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                wall_clock64() - t_start > 500000000ull) {
                __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.aborted = true;
                return;
            }
        }
    }
}

// wave-level: two runs of consecutive rows (NA rows from rowA, NB from rowB, granule stride 64) polled together
template <int NA, int NB>
__device__ __forceinline__ void wait_two_runs(Xg2 &x, const u64 *rowA, const u64 *rowB, unsigned int tag, unsigned lane,
                                              float (&outA)[NA], float (&outB)[NB])
{
    unsigned int spins = 0;
    unsigned long long t_start = 0;
    for (;;) {
        u64 ga[NA], gb[NB];
#pragma unroll
        for (int k = 0; k < NA; ++k) ga[k] = ld_gran(rowA + (size_t)k * 64 + lane);
#pragma unroll
        for (int k = 0; k < NB; ++k) gb[k] = ld_gran(rowB + (size_t)k * 64 + lane);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NA; ++k) ok = ok && ((unsigned int)(ga[k] >> 32) == tag);
#pragma unroll
        for (int k = 0; k < NB; ++k) ok = ok && ((unsigned int)(gb[k] >> 32) == tag);
#pragma unroll
        for (int k = 0; k < NA; ++k) outA[k] = __uint_as_float((unsigned int)ga[k]);
#pragma unroll
        for (int k = 0; k < NB; ++k) outB[k] = __uint_as_float((unsigned int)gb[k]);
        if (__all(ok) || x.aborted) {
            asm volatile("" ::: "memory");
            return;
        }
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0) {
            if (t_start == 0) t_start = wall_clock64();
            if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                wall_clock64() - t_start > 500000000ull) {
                __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.aborted = true;
                return;
            }
        }
    }
}

// wave-level: wait until the LDS word *p has reached `want` (written by the partner wave of the pair)
__device__ __forceinline__ void wait_lds_ge(Xg2 &x, const int *p, int want)
{
    unsigned int spins = 0;
    unsigned long long t_start = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want && !x.aborted) {
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 1023u) == 0) {
            if (t_start == 0) t_start = wall_clock64();
            if (__hip_atomic_load(x.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                wall_clock64() - t_start > 500000000ull) {
                __hip_atomic_store(x.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.aborted = true;
            }
        }
    }
    asm volatile("" ::: "memory");
}
// lanes of ONE wave exchanging data through LDS: order the accesses (the hardware executes a wave's LDS operations in
// issue order; this keeps the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int V>
struct IC { static constexpr int value = V; };   // compile-time wave role (0: y-wave, 1: a-wave) of the hot lambdas

__device__ __forceinline__ void act_grad_fast2(float y, float &da, float &dl)
{
    const float s = y - 0.5f;
    const float d = 1.0f + fabsf(s);
    const float rd = fast_rcp(d);
    da = rd * rd;
    dl = (s < 0.0f) ? rd : fast_rcp((1.0f + s) * (1.0f + 2.0f * s));
}

enum { F_BASE = 0, F_H0 = 1, F_DP = 2, F_FIX = 3 };

// row st-1 of the Dormand-Prince tableau (dopri5.py:5-30) as instruction literals: the hot loop reads no table
__device__ __forceinline__ void dp_beta_row(int st, float (&b)[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = 0.f;
    switch (st) {
        case 1: b[0] = (float)(1.0 / 5); break;
        case 2: b[0] = (float)(3.0 / 40); b[1] = (float)(9.0 / 40); break;
        case 3: b[0] = (float)(44.0 / 45); b[1] = (float)(-56.0 / 15); b[2] = (float)(32.0 / 9); break;
        case 4: b[0] = (float)(19372.0 / 6561); b[1] = (float)(-25360.0 / 2187); b[2] = (float)(64448.0 / 6561);
                b[3] = (float)(-212.0 / 729); break;
        case 5: b[0] = (float)(9017.0 / 3168); b[1] = (float)(-355.0 / 33); b[2] = (float)(46732.0 / 5247);
                b[3] = (float)(49.0 / 176); b[4] = (float)(-5103.0 / 18656); break;
        case 6: b[0] = (float)(35.0 / 384); b[1] = 0.0f; b[2] = (float)(500.0 / 1113); b[3] = (float)(125.0 / 192);
                b[4] = (float)(-2187.0 / 6784); b[5] = (float)(11.0 / 84); break;
        default: break;
    }
}
// c_err = c_sol - c_error of the embedded pair (dopri5.py), entries 0..5 (entry 6 = -1/60 is applied with k7)
__device__ __forceinline__ void dp_cerr_row(float (&e)[6])
{
    e[0] = (float)(35.0 / 384 - 1951.0 / 21600); e[1] = 0.0f; e[2] = (float)(500.0 / 1113 - 22642.0 / 50085);
    e[3] = (float)(125.0 / 192 - 451.0 / 720); e[4] = (float)(-2187.0 / 6784 - -12231.0 / 42400);
    e[5] = (float)(11.0 / 84 - 649.0 / 6300);
}

template <int HT, int NP2>
__global__ __launch_bounds__(128 * NP2) void k1_solve_adj2(Net net, D1 d, W1 w, SolveCfg cfg, const double *__restrict__ t,
                                                     const float *__restrict__ y_saved,
                                                     const float *__restrict__ grad_y, float *adj_y0, int *status,
                                                     int *nfe_out, int *nsteps_out, int want_grads, long long PP,
                                                     int stagger_ticks, int prof_wave)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: tell the compiler so
    const int side = wv >= NP2 ? 1 : 0;     // 0: y-wave, 1: a-wave
    // waves w and w + 4 share a SIMD: the a-wave there belongs to a pair of the OTHER half of the workgroup
    const int pr = side ? (wv - NP2 + NP2 / 2) % NP2 : wv;
    const int grp = blockIdx.x / d.G, gt = blockIdx.x % d.G;
    const int blk0 = gt * d.NB;
    const int nbl = min(d.NB, d.nblk - blk0);
    const int N = d.N, H = d.H, B = d.B, T = d.T, Bt = d.Bt, ntg = d.ntg, G = d.G, TPW = d.TPW;
    const int BLKF = blk_floats_ch(HT, H);
    const int RGOFF = BLKF - 32;
    const bool shared = cfg.control == PHX_CTRL_SHARED;
    constexpr int F4 = 4 * HT, F2 = 2 * HT;
    char *ctlbase = reinterpret_cast<char *>(lds + (long long)d.NB * BLKF);
    int *flag_ag = reinterpret_cast<int *>(ctlbase);               // [NP2] gathers finished by the a-wave of a pair
    int *flag_ps = flag_ag + NP2;                                  // [NP2][2] pair rendezvous counters
    int *flag_ys = flag_ag + 3 * NP2_MAX;                          // [NP2] last sweep whose y stage tiles are complete
    unsigned long long *tacc = reinterpret_cast<unsigned long long *>(ctlbase + 256);
    const WC2 c = carve_wc2(ctlbase + ADJ2_FLAG_BYTES + (size_t)wv * ADJ2_WC_PER_TRAJ * 16 * TPW, 16 * TPW);
    const int RH = ntg * F4 * 4;            // hidden rows of one exchange: per tile [u | v | dz_u | dz_p] x HT x 4
    const int R = RH + 2 * ntg;             // partial rows: + one norm row per tile and side
    const int RZ = RH + 4 * ntg;            // reduced rows: the norm rows are double buffered by exchange parity
    u64 *part = w.part + (long long)grp * G * R * 64;
    u64 *zb = w.zbuf + (long long)grp * RZ * 64;
    Xg2 x{w.abort_flag, false};
    unsigned int tagH = 0u, tagN = 0u;
    int n_gather = 0, n_sync = 0;           // pair protocol counters (same sequence in both waves of a pair)
    int n_sweep = 0, last_out_sweep = 0;    // sweeps started / the last one that formed a stage input
    SegTimer tm;
    tm.acc = tacc;
    tm.on = w.prof != nullptr && wv == prof_wave && lane == 0;   // diagnostic: one wave of the workgroup keeps the segment timers
    if (tm.on) {
        for (int k = 0; k < 16; ++k) tacc[k] = 0;
        tm.last = wall_clock64();
        tacc[15] = (unsigned long long)clock64();   // diagnostic: shader clock of the whole kernel (slot 15)
    }

    if (tid < 64) flag_ag[tid] = 0;         // flag_ag + flag_ps
    stage_images(w.wimg, lds, blk0, nbl, 0, 1, BLKF);
    __syncthreads();                        // the ONLY workgroup barrier: from here on every wave runs on its own
    if (pr * TPW >= ntg) return;            // pair without a tile (single small group)

    const int offR = li * LROW + gmap(lq, 0);
    int offC[2];
    offC[0] = 4 * lq * LROW + gmapC(li, 0);
    offC[1] = 4 * lq * LROW + gmapC(li, 1);
    const int tiles_wg = ntg * d.NB;
    float *wgbase = w.scratch + (long long)blockIdx.x * NVEC_ADJ2 * tiles_wg * 512;
    const unsigned lane8 = lane * 8;
    auto tptr = [&](int v, int ttl, int bl) -> float * {   // (uniform base + uniform tile offset) + 32-bit lane offset
        float *tb = wgbase + (unsigned)((v * tiles_wg + ttl * d.NB + bl) * 512);
        return tb + lane8;
    };
    // wave-private transposed hidden rows of the seven stage slots: [wave][tile of the wave][slot][F2][64] float4
    float *hqbase = w.hq + ((long long)blockIdx.x * 2 * NP2 + wv) * TPW * 7 * F2 * 256;
    auto hqp = [&](int s, int slot, int f) -> float4 * {
        return reinterpret_cast<float4 *>(hqbase + ((unsigned)(((s * 7 + slot) * F2 + f) * 256) + (unsigned)lane * 4));
    };
    float *dth = w.dtheta + (long long)(grp * NP2 + pr) * PP;   // this pair's parameter-gradient partial
    const long long oWs = 0, oWp = (long long)H * N, oWa = 2LL * H * N, og = 4LL * H * N, obs = og + N, obp = obs + H;
    const int nts = min(TPW, ntg - pr * TPW);   // tiles of this wave

    // ---- controllers of this wave's tiles (lane li <-> trajectory li of the tile; the four lq copies agree)
    for (int s = 0; s < nts; ++s) {
        const int i = s * 16 + li;
        const int b = grp * Bt + (pr * TPW + s) * 16 + li;
        const bool vb = b < B;
        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : (vb ? b : 0));
        float sg = 1.0f;
        int st = PHX_OK;
        if (T >= 2) {
            sg = (tb[1] < tb[0]) ? -1.0f : 1.0f;
            for (int k = 0; k + 1 < T; ++k)
                if (!((double)sg * tb[k + 1] > (double)sg * tb[k])) st = PHX_ERR_BAD_ARG;
        }
        if (lq == 0) {
            c.sgn[i] = sg; c.st[i] = vb ? st : PHX_OK; c.nsteps[i] = 0; c.nfe[i] = 0;
            c.done[i] = (!vb || st != PHX_OK) ? 1 : 0;
            c.accept[i] = 0; c.fin[i] = 0; c.nsiv[i] = 0;
            // padding trajectories (b >= B) never get a step size: with dt = 0 they stay at their fill state
            // (y = 0.5, a = 0), which keeps every value of their MFMA columns finite without masks in the sweeps
            c.dt[i] = 0.0; c.dtf[i] = 0.f; c.dtp[i] = 0.f; c.h0f[i] = 0.f; c.d1[i] = 0.f; c.xfin[i] = 1.0;
            c.rk_t0[i] = 0.0; c.rk_t1[i] = 0.0;
            for (int j = 0; j < 8; ++j) c.wq[i * 8 + j] = 0.f;
        }
    }
    wave_lds_sync();
    // ---- terminal state (adjoint.py:86-87): y-waves load y(t_end), a-waves dL/dy(t_end)
    for (int s = 0; s < nts; ++s) {
        const int ttl = pr * TPW + s;
        const int b = grp * Bt + ttl * 16 + li;
        for (int bl = 0; bl < nbl; ++bl) {
            float v8[8];
            const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
            const long long ro = (long long)(T - 1) * d.BN + (long long)b * N;
            row_load8(side ? grad_y : y_saved, ro, g0, N, b < B, side ? 0.f : 0.5f, v8);
            store8(tptr(vX0(side), ttl, bl), v8);
        }
    }
    tm.mark(6);
    // stagger: the second half of the pairs starts late, so that the two waves of a SIMD are out of phase
    if (stagger_ticks > 0 && pr >= NP2 / 2 && !shared) {
        const unsigned long long t0 = wall_clock64();
        while (wall_clock64() - t0 < (unsigned long long)stagger_ticks) __builtin_amdgcn_s_sleep(8);
    }

    // options["step_size"]: every interval has its own step grid anchored at its start (adjoint.py:137-154 calls odeint
    // per interval); c.nsiv = steps taken in the interval, c.rk_t0 / rk_t1 / dtf = the running step; cfg.max_steps is a
    // budget of grid steps per interval, as it is per interval for dopri5
    const bool stepped = cfg.method != PHX_DOPRI5 && cfg.step > 0.0;
    auto dt_rev = [&](int i, int b, int iv) -> float {   // reversed pair (-t_i, -t_{i-1}) of the fixed grid
        if (stepped) return c.dtf[i];
        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : min(b, B - 1));
        const double sg = (double)c.sgn[i];
        const double u0 = -sg * tb[iv], u1 = -sg * tb[iv - 1];
        return cfg.t_is_f32 ? ((float)u1 - (float)u0) : (float)(u1 - u0);
    };
    // rendezvous of the two waves of a pair; everything either wave stored before it is visible to both after it
    auto pair_sync = [&]() {
        n_sync += 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(&flag_ps[pr * 2 + side], n_sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        wait_lds_ge(x, &flag_ps[pr * 2 + (1 - side)], n_sync);
    };

    // Reduction of the exchange rows [u0, u1) (one tile, one side) that THIS workgroup owns (row u belongs to
    // workgroup u % G): the members' partial rows are summed in member order (deterministic), `post` applied, the
    // reduced row published at granule offset `zoff(u)` with the exchange tag.
    auto reduce_owned = [&](int u0, int u1, unsigned int tag, auto zoff, auto post) {
        const int first = u0 + ((gt - u0 % G) + G) % G;
        if (G <= 16 && HT == 3) {
            // few members, narrow hidden layer (the in-silico shape: 2-3 owned rows per range): every owned row's members
            // in ONE batch of loads -- these launches are bound by the round trips, not by bytes
            constexpr int NRW = 3;
            for (int u = first; u < u1; u += NRW * G) {
                const int nr = min(NRW, (u1 - u + G - 1) / G);
                float v[NRW][16];
                wait_members_rows<NRW, 16>(x, part + (unsigned)(u * 64), (unsigned)(G * 64), (unsigned)(R * 64), nr, G, tag,
                                           lane, v);
#pragma unroll
                for (int r = 0; r < NRW; ++r) {
                    if (r >= nr) break;
                    float tot = 0.f;
#pragma unroll
                    for (int m = 0; m < 16; ++m) tot += (m < G) ? v[r][m] : 0.f;
                    st_gran(zb + zoff(u + r * G), lane, post(u + r * G, tot), tag);
                }
            }
            return;
        }
        for (int u = first; u < u1; u += G) {
            float tot = 0.f;
            const u64 *row0 = part + (unsigned)(u * 64);
            if (G <= 16) {          // every member's row in one batch of loads (member order => deterministic sum)
                float v[16];
                wait_members<16>(x, row0, (unsigned)(R * 64), G, tag, lane, v);
#pragma unroll
                for (int m = 0; m < 16; ++m) tot += (m < G) ? v[m] : 0.f;
            } else {
                for (int m0 = 0; m0 < G; m0 += 32) {
                    const int nv = min(32, G - m0);
                    float v[32];
                    wait_members<32>(x, row0 + (size_t)m0 * (R * 64), (unsigned)(R * 64), nv, tag, lane, v);
#pragma unroll
                    for (int m = 0; m < 32; ++m) tot += (m < nv) ? v[m] : 0.f;
                }
            }
            st_gran(zb + zoff(u), lane, post(u, tot), tag);
        }
    };
    auto hoff = [&](int ttl, int f4, int r) -> unsigned { return (unsigned)(((ttl * F4 + f4) * 4 + r) * 64); };

    // -----------------------------------------------------------------------------------------------------------
    // One sweep over this wave's tiles (SC: compile-time role of the calling wave).
    //   sin  >= 0: the reduced hidden rows of stage slot `sin` (exchange tagH) feed P2' -> K[sin], norm partials by
    //              rmode (1: d0, d1 of misc.py:62-67; 2: d2 of misc.py:74-77; 3: error ratio, misc.py:89-91)
    //   sout >= 0: the stage input of slot `sout` is formed (fmode), stored, and contracted (P1') into the partial
    //              rows of a NEW exchange; the rows this wave owns are reduced right away
    // Block pipeline: the tiles of block b+1 are requested, then P1'(b) and P2'(b+1) -- which need no tile data --
    // run while they are in flight; block b+1 is finished (k, norms, next input, activations) when they arrive.
    // -----------------------------------------------------------------------------------------------------------
    auto sweep = [&](auto SC, auto STC, int sin_, int rmode_, int sout_, int fmode_, int iv) {
        constexpr int SIDE = decltype(SC)::value;
        // HOT > 0: the fused dopri5 sweep "stage HOT -> input of stage HOT + 1, no norms" with its shape known at compile
        // time: no branch inside a gene block, so the MFMA and vector streams of a block can be interleaved
        constexpr int HOT = decltype(STC)::value;
        const int sin = HOT ? HOT : sin_, sout = HOT ? HOT + 1 : sout_, fmode = HOT ? (int)F_DP : fmode_, rmode = HOT ? 0 : rmode_;
        tm.mark(0);
        n_sweep += 1;
        const int ys_needed = last_out_sweep;   // the sweep that wrote the stage tiles this one consumes
        if (sout >= 0) last_out_sweep = n_sweep;
        const unsigned int tagIn = tagH;
        if (sout >= 0) tagH += 1u;
        const unsigned int tagOut = tagH;
        if (rmode != 0) tagN += 1u;
        const bool fused = sin >= 0 && sout == sin + 1 && (fmode == F_DP || fmode == F_FIX);
        const int st = sout;                                                               // stage being formed
        const int nk = (sout < 0 || fmode == F_BASE) ? 0 : (fmode == F_H0 ? 1 : sout);     // k tiles of the input
        const int nload = fused ? nk - 1 : nk;                                             // ... read from memory
        float brow[6], erow[6];
        dp_beta_row(fmode == F_DP ? st : 0, brow);
        dp_cerr_row(erow);
        const float rtol = cfg.rtol, atol = cfg.atol;
        const int method = cfg.method;
        for (int s = 0; s < nts; ++s) {
            const int ttl = pr * TPW + s;
            float hr[F2][4];   // y-wave: z_u | z_p        a-wave: du | dv
            if (sin >= 0) {
                // the tile's reduced rows of this wave's sections are consecutive: few large batches of loads
                if (SIDE == 0) {
                    constexpr int FB = (HT == 3) ? 6 : 8;      // hidden tiles per batch (z_u | z_p are rows [0, 2HT))
#pragma unroll
                    for (int f0 = 0; f0 < F2; f0 += FB) {
                        float v[FB * 4];
                        wait_members<FB * 4>(x, zb + hoff(ttl, f0, 0), 64u, FB * 4, tagIn, lane, v);
#pragma unroll
                        for (int k = 0; k < FB * 4; ++k) hr[f0 + (k >> 2)][k & 3] = v[k];
                    }
                } else {
                    // du | dz_p are the consecutive rows [2HT, 4HT) x 4 of the tile, z_p the rows [HT, 2HT) x 4
                    if (HT == 3) {   // everything in one batch of loads
                        float vd[F2 * 4], vp[HT * 4];
                        wait_two_runs<F2 * 4, HT * 4>(x, zb + hoff(ttl, 2 * HT, 0), zb + hoff(ttl, HT, 0), tagIn, lane, vd, vp);
#pragma unroll
                        for (int kk = 0; kk < HT * 4; ++kk) {
                            hr[kk >> 2][kk & 3] = vd[kk];
                            hr[HT + (kk >> 2)][kk & 3] = vd[HT * 4 + kk] * vp[kk];
                        }
                    } else {
                        constexpr int FB = 4;      // hidden tiles per batch
#pragma unroll
                        for (int f0 = 0; f0 < HT; f0 += FB) {
                            float vd[FB * 4], vz[FB * 4], vp[FB * 4];
                            wait_two_runs<FB * 4, FB * 4>(x, zb + hoff(ttl, 2 * HT + f0, 0), zb + hoff(ttl, 3 * HT + f0, 0), tagIn, lane, vd, vz);
                            wait_members<FB * 4>(x, zb + hoff(ttl, HT + f0, 0), 64u, FB * 4, tagIn, lane, vp);
#pragma unroll
                            for (int kk = 0; kk < FB * 4; ++kk) {
                                hr[f0 + (kk >> 2)][kk & 3] = vd[kk];
                                hr[HT + f0 + (kk >> 2)][kk & 3] = vz[kk] * vp[kk];
                            }
                        }
                    }
                    // the partner's stage input y_s (written in its previous forming sweep) is complete
                    wait_lds_ge(x, &flag_ys[pr], ys_needed);
                    // the y-wave of the pair may now let the z_p rows of this exchange be overwritten
                    n_gather += 1;
                    if (lane == 0)
                        __hip_atomic_store(&flag_ag[pr], n_gather, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (SIDE == 0) n_gather += 1;
                if (want_grads) {   // transposed copies for the quadrature (operands of products over trajectories)
#pragma unroll
                    for (int f = 0; f < F2; ++f) {
                        float o[4];
                        xpose4(hr[f], o, lane);
                        *hqp(s, sin, f) = make_float4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
            if (s == 0) tm.mark(4);
            const int i = s * 16 + li;
            const int b = grp * Bt + ttl * 16 + li;
            const float sg = c.sgn[i];
            const float dte = c.dtf[i];       // step size of the running dopri5 step (error estimate, rmode 3)
            float dtl = 0.f;                  // step size that forms the next stage input
            if (fmode == F_H0) dtl = c.h0f[i];
            else if (fmode == F_DP) dtl = c.dtf[i];
            else if (fmode == F_FIX) dtl = dt_rev(i, b, iv);
            f32x4 acc[F2];
#pragma unroll
            for (int f = 0; f < F2; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float r0 = 0.f, r1 = 0.f;
            float xs[8], ysx[8], x0v[8], ev[8], kq[6][8], p0[8], p1[8];
            // ---- requests of one block: everything it needs, issued back to back
            auto issue = [&](int bl) {
                if (sin >= 0) {
                    load8(tptr(vXS(SIDE, sin), ttl, bl), xs);
                    if (SIDE == 1) load8(tptr(vXS(0, sin), ttl, bl), ysx);   // the a-wave differentiates at y_s
                    if (rmode == 3) load8(tptr(vE(SIDE), ttl, bl), ev);
                }
                if (sout >= 0 || rmode >= 2) load8(tptr(vX0(SIDE), ttl, bl), x0v);
                if (rmode == 2) load8(tptr(vK(SIDE, 0), ttl, bl), kq[0]);
#pragma unroll
                for (int kk = 0; kk < 5; ++kk)
                    if (kk < nload) {
                        if (fmode == F_DP && st == 6 && kk == 1) zero8(kq[kk]);   // beta_62 = c_err2 = 0
                        else load8(tptr(vK(SIDE, kk), ttl, bl), kq[kk]);
                    }
            };
            // ---- P2' of one block: expansion back to genes (needs the hidden rows and LDS only)
            auto p2 = [&](int bl, float (&o0)[8], float (&o1)[8]) {
                const float *Wb = lds + (long long)bl * BLKF;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const float *Wc = Wb + offC[s2];
                    f32x4 a0 = (f32x4){0.f, 0.f, 0.f, 0.f}, a1 = a0;
                    if (SIDE == 0) {   // j = Wa z  (z_u rows then z_p rows)
#pragma unroll
                        for (int f2 = 0; f2 < F2; ++f2) {
                            const int rb = (f2 < HT) ? 2 * H + 16 * f2 : 3 * H + 16 * (f2 - HT);
#pragma unroll
                            for (int r = 0; r < 4; ++r) a0 = mfma4(Wc[(rb + r) * LROW], hr[f2][r], a0);
                        }
                    } else {           // a~ = Ws^T du, l~ = Wp^T dv
#pragma unroll
                        for (int f = 0; f < HT; ++f)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                a0 = mfma4(Wc[(16 * f + r) * LROW], hr[f][r], a0);
                                a1 = mfma4(Wc[(H + 16 * f + r) * LROW], hr[HT + f][r], a1);
                            }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) { o0[4 * s2 + r] = a0[r]; o1[4 * s2 + r] = a1[r]; }
                }
            };
            if (!HOT) issue(0);
            if (sin >= 0) p2(0, p0, p1);
            if (!HOT) tm.mark(14);
            if constexpr (HOT > 0) {
                // ---------------------------------------------------------------------------------------------------
                // Hot form (fused dopri5 stage, shape known at compile time): the vector work that finishes ELEMENT
                // j + 1 of the block (k, next stage input, activations -- all elementwise over the lane's eight genes)
                // is cut into slices and issued one slice per MFMA of element j's group of P1' (one B operand = one
                // element).  The scheduler is fenced after every (MFMA, slice, LDS read) triple, so the matrix pipe runs
                // under the vector stream instead of after it.  P2'(b+1) then covers the tile requests of block b + 1.
                // ---------------------------------------------------------------------------------------------------
                constexpr int ST = HOT + 1;              // stage whose input is formed
                // With 512 registers per wave (two pairs per workgroup) the tile registers are double buffered: the
                // requests of block b + 1 go out BEFORE block b is processed and have a whole block of cover.
                constexpr int NSET = (NP2 == 2) ? 2 : 1;
                float cf[6], ce[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) { cf[k] = brow[k] * dtl; ce[k] = dtl * erow[k]; }
                float hxs[NSET][8], hys[NSET][8], hx0[NSET][8], hkq[NSET][5][8];
                auto issue_h = [&](auto PC, int bl) {
                    constexpr int P = decltype(PC)::value;
                    load8(tptr(vXS(SIDE, sin), ttl, bl), hxs[P]);
                    if (SIDE == 1) load8(tptr(vXS(0, sin), ttl, bl), hys[P]);   // the a-wave differentiates at y_s
                    load8(tptr(vX0(SIDE), ttl, bl), hx0[P]);
#pragma unroll
                    for (int kk = 0; kk < ST - 1; ++kk) {
                        if (ST == 6 && kk == 1) zero8(hkq[P][kk]);   // beta_62 = c_err2 = 0
                        else load8(tptr(vK(SIDE, kk), ttl, bl), hkq[P][kk]);
                    }
                };
                auto body = [&](auto PC, int bl) {
                    constexpr int P = decltype(PC)::value;
                    // unconditional (the last block re-requests itself): a request under a condition makes the compiler
                    // merge "loaded" and "old" register versions with copies, which wait for the loads at once
                    if (NSET == 2) issue_h(IC<(NSET == 2 ? 1 - P : P)>{}, min(bl + 1, nbl - 1));
#ifdef PHX_PROF_BLOCKS   // per-block marks: diagnostic build only (run-time branches inside the block loop cost 1-2 %)
                    if (NSET == 2 && tm.on) {   // diagnostic: how long this block's tiles (requested one block ago) are still out
                        constexpr int NLD = 2 * (2 + (SIDE == 1 ? 1 : 0) + (ST - 1) - (ST == 6 ? 1 : 0));
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
                        tm.mark(12);
                    }
#endif
                    const float *Wb = lds + (long long)bl * BLKF;
                    const float *rg = Wb + RGOFF;
                    const float *Wr = Wb + offR;
                    float kx[8], xn[8], bop[8], bop2[8], e8[8];
                    float tS[8], tD[8], tR[8], tA[8], tM[8], tRR[8], tDA[8], tDL[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) tRR[j] = rg[gmap(lq, j)];   // one LDS round trip per block, not one per element
                    // one slice of the vector work of element j
                    auto slice = [&](int j, int k) {
                        if (SIDE == 0) {
                            if (k == 0) {
                                kx[j] = -sg * (tRR[j] * (p0[j] - hxs[P][j]));
                            } else if (k == 1) {
                                float sacc = 0.f;
#pragma unroll
                                for (int kk = 0; kk < ST - 1; ++kk) sacc += hkq[P][kk][j] * cf[kk];
                                sacc += kx[j] * cf[ST - 1];
                                xn[j] = hx0[P][j] + sacc;
                                if (ST == 6) {
                                    float ee = 0.f;
#pragma unroll
                                    for (int kk = 0; kk < 5; ++kk) ee += hkq[P][kk][j] * ce[kk];
                                    e8[j] = ee + kx[j] * ce[5];
                                }
                            } else if (k == 2) {
                                tS[j] = xn[j] - 0.5f;
                                tD[j] = 1.0f + fabsf(tS[j]);
                                tR[j] = __builtin_amdgcn_rcpf(tD[j]);
                            } else if (k == 3) {
                                tR[j] = fmaf(fmaf(-tD[j], tR[j], 1.0f), tR[j], tR[j]);
                                tA[j] = tS[j] * tR[j];
                                float sm = 1.0f / 13.0f;
                                const float x = -tA[j];
                                sm = fmaf(sm, x, 1.0f / 12.0f); sm = fmaf(sm, x, 1.0f / 11.0f); sm = fmaf(sm, x, 1.0f / 10.0f);
                                tM[j] = sm;
                            } else if (k == 4) {
                                float sm = tM[j];
                                const float x = -tA[j];
                                sm = fmaf(sm, x, 1.0f / 9.0f); sm = fmaf(sm, x, 1.0f / 8.0f); sm = fmaf(sm, x, 1.0f / 7.0f);
                                sm = fmaf(sm, x, 1.0f / 6.0f); sm = fmaf(sm, x, 1.0f / 5.0f);
                                tM[j] = sm;
                            } else if (k == 5) {
                                float sm = tM[j];
                                const float x = -tA[j];
                                sm = fmaf(sm, x, 1.0f / 4.0f); sm = fmaf(sm, x, 1.0f / 3.0f); sm = fmaf(sm, x, 0.5f);
                                sm = fmaf(sm, x, 1.0f);
                                const float small = tA[j] * sm;
                                const float big = __builtin_amdgcn_logf(1.0f + tA[j]) * 0.69314718055994531f;
                                bop[j] = tA[j];
                                bop2[j] = (fabsf(tA[j]) < 0.25f) ? small : big;
                            }
                        } else {
                            if (k == 0) {
                                tS[j] = hys[P][j] - 0.5f;
                                tD[j] = 1.0f + fabsf(tS[j]);
                                tR[j] = __builtin_amdgcn_rcpf(tD[j]);
                            } else if (k == 1) {
                                tR[j] = fmaf(fmaf(-tD[j], tR[j], 1.0f), tR[j], tR[j]);
                                tDA[j] = tR[j] * tR[j];
                                tM[j] = (1.0f + tS[j]) * (1.0f + 2.0f * tS[j]);
                                tA[j] = __builtin_amdgcn_rcpf(tM[j]);
                            } else if (k == 2) {
                                const float r2 = fmaf(fmaf(-tM[j], tA[j], 1.0f), tA[j], tA[j]);
                                tDL[j] = (tS[j] < 0.0f) ? tR[j] : r2;
                            } else if (k == 3) {
                                kx[j] = sg * ((p0[j] * tDA[j] + p1[j] * tDL[j]) - hxs[P][j] * tRR[j]);
                            } else if (k == 4) {
                                float sacc = 0.f;
#pragma unroll
                                for (int kk = 0; kk < ST - 1; ++kk) sacc += hkq[P][kk][j] * cf[kk];
                                sacc += kx[j] * cf[ST - 1];
                                xn[j] = hx0[P][j] + sacc;
                                if (ST == 6) {
                                    float ee = 0.f;
#pragma unroll
                                    for (int kk = 0; kk < 5; ++kk) ee += hkq[P][kk][j] * ce[kk];
                                    e8[j] = ee + kx[j] * ce[5];
                                }
                            } else if (k == 5) {
                                bop[j] = xn[j] * tRR[j];
                            }
                        }
                    };
                    // A operand m of element j's MFMA group: y-wave u rows | v rows, a-wave dz_u rows | dz_p rows
                    auto a_op = [&](int j, int m) -> float {
                        const int row = SIDE == 0 ? (m < HT ? m * 16 : H + (m - HT) * 16)
                                                  : (m < HT ? 2 * H + 16 * m : 3 * H + 16 * (m - HT));
                        return Wr[row * LROW + j];
                    };
                    float Ac[F2], An[F2];
#pragma unroll
                    for (int k = 0; k < 6; ++k) slice(0, k);            // element 0: nothing to hide it under
#pragma unroll
                    for (int m = 0; m < F2; ++m) Ac[m] = a_op(0, m);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
#pragma unroll
                        for (int m = 0; m < F2; ++m) {
                            acc[m] = mfma4(Ac[m], (SIDE == 0 && m >= HT) ? bop2[j] : bop[j], acc[m]);
                            if (j + 1 < 8) {
                                if (m < 6) slice(j + 1, m);
                                An[m] = a_op(j + 1, m);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
#pragma unroll
                        for (int m = 0; m < F2; ++m) Ac[m] = An[m];
                    }
                    store8(tptr(vK(SIDE, sin), ttl, bl), kx);
                    store8(tptr(vXS(SIDE, sout), ttl, bl), xn);
                    if (ST == 6) store8(tptr(vE(SIDE), ttl, bl), e8);
                    __builtin_amdgcn_sched_barrier(0);
                    if (NSET == 1) issue_h(IC<P>{}, min(bl + 1, nbl - 1));
                    if (bl + 1 < nbl) {
                        p2(bl + 1, p0, p1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                };
                issue_h(IC<0>{}, 0);
                tm.mark(14);   // hot: rows copied for the quadrature, first requests, P2'(0)
                for (int bl = 0; bl < nbl; bl += 2) {
                    body(IC<0>{}, bl);
                    if (bl + 1 < nbl) body(IC<(NSET == 2 ? 1 : 0)>{}, bl + 1);
                }
                tm.mark(13);   // hot: the pipelined block loop
            } else {
                for (int bl = 0; bl < nbl; ++bl) {
                    const float *Wb = lds + (long long)bl * BLKF;
                    const float *rg = Wb + RGOFF;
                    float kx[8], bop[8], bop2[8];
                    // HOT: no conditional code below, the last block repeats itself as its own successor (clamped index)
                    const bool has_next = HOT ? true : (bl + 1 < nbl);
                    const int bn = min(bl + 1, nbl - 1);
#ifdef PHX_PROF_BLOCKS   // per-block marks: diagnostic build only (run-time branches inside the block loop cost 1-2 %)
                    if (!HOT && tm.on) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tm.mark(12); }   // diagnostic: tile wait
#endif
                    if (sin >= 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float rr = rg[gmap(lq, j)];
                            if (SIDE == 0) kx[j] = -sg * (rr * (p0[j] - xs[j]));
                            else {
                                float da, dl;
                                act_grad_fast2(ysx[j], da, dl);
                                kx[j] = sg * ((p0[j] * da + p1[j] * dl) - xs[j] * rr);
                            }
                        }
                        store8(tptr(vK(SIDE, sin), ttl, bl), kx);
                        if (rmode != 0) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const int gene = (blk0 + bl) * 32 + gmap(lq, j);
                                if (!((b < B) && (gene < N))) continue;
                                if (rmode == 1) {
                                    const float sc = atol + fabsf(xs[j]) * rtol;
                                    const float q0 = xs[j] / sc, q1 = kx[j] / sc;
                                    r0 += q0 * q0; r1 += q1 * q1;
                                } else if (rmode == 2) {
                                    const float sc = atol + fabsf(x0v[j]) * rtol;
                                    const float q0 = (kx[j] - kq[0][j]) / sc;
                                    r0 += q0 * q0;
                                } else {
                                    const float e = ev[j] + kx[j] * (dte * DP_CERR[6]);
                                    const float tol = atol + rtol * fmaxf(fabsf(x0v[j]), fabsf(xs[j]));
                                    const float q0 = e / tol;
                                    r0 += q0 * q0;
                                }
                            }
                        }
                    }
                    if (sout >= 0) {
                        // ---- next stage input (rk_common.py:62-66, fixed_grid.py, rk_common.py:96-103), fp32, k ascending
                        float xn[8];
                        if (fmode == F_BASE) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) xn[j] = x0v[j];
                        } else {
                            if (fused) {
#pragma unroll
                                for (int kk = 0; kk < 6; ++kk)
                                    if (kk == nk - 1) {
#pragma unroll
                                        for (int j = 0; j < 8; ++j) kq[kk][j] = kx[j];
                                    }
                            }
                            if (fmode == F_H0) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + dtl * kq[0][j];
                            } else if (fmode == F_DP) {
                                float sacc[8];
#pragma unroll
                                for (int j = 0; j < 8; ++j) sacc[j] = 0.f;
#pragma unroll
                                for (int kk = 0; kk < 6; ++kk)
                                    if (kk < st) {
                                        const float cf = brow[kk] * dtl;
#pragma unroll
                                        for (int j = 0; j < 8; ++j) sacc[j] += kq[kk][j] * cf;
                                    }
#pragma unroll
                                for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + sacc[j];
                                if (st == 6) {   // all k tiles of the step but the last are in registers: error estimate so far
                                    float e8[8];
#pragma unroll
                                    for (int j = 0; j < 8; ++j) e8[j] = 0.f;
#pragma unroll
                                    for (int kk = 0; kk < 6; ++kk) {
                                        const float ce = dtl * erow[kk];
#pragma unroll
                                        for (int j = 0; j < 8; ++j) e8[j] += kq[kk][j] * ce;
                                    }
                                    store8(tptr(vE(SIDE), ttl, bl), e8);
                                }
                            } else if (method == PHX_MIDPOINT) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + kq[0][j] * (0.5f * dtl);
                            } else {   // rk4 = 3/8 rule
                                const float third = (float)(1.0 / 3.0);
                                if (st == 1) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + (dtl * kq[0][j]) * third;
                                } else if (st == 2) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + dtl * (kq[1][j] - kq[0][j] * third);
                                } else {
#pragma unroll
                                    for (int j = 0; j < 8; ++j) xn[j] = x0v[j] + dtl * ((kq[0][j] - kq[1][j]) + kq[2][j]);
                                }
                            }
                        }
                        store8(tptr(vXS(SIDE, sout), ttl, bl), xn);
                        // ---- B operands of P1'.  No masks: a padded gene keeps (y, a) = (0.5, 0) for the whole solve (its weight
                        // columns and relu(g) are zero in the LDS image), where a(y) = l(y) = q = 0; a padding trajectory only
                        // feeds its own MFMA column.
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if (SIDE == 0) act_pair_fast(xn[j], bop[j], bop2[j]);
                            else bop[j] = xn[j] * rg[gmap(lq, j)];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS   // per-block marks: diagnostic build only (run-time branches inside the block loop cost 1-2 %)
                    if (!HOT) tm.mark(13);   // finishing a block: k, norms, next input, activations
#endif
                    if (has_next) issue(bn);
                    if (sout >= 0) {
                        // ---- P1': contraction over this block's genes
                        const float *Wr = Wb + offR;
                        if (SIDE == 0) {
#pragma unroll
                            for (int j = 0; j < 8; ++j)
#pragma unroll
                                for (int f = 0; f < HT; ++f) {
                                    acc[f] = mfma4(Wr[f * 16 * LROW + j], bop[j], acc[f]);
                                    acc[HT + f] = mfma4(Wr[(H + f * 16) * LROW + j], bop2[j], acc[HT + f]);
                                }
                        } else {
#pragma unroll
                            for (int j = 0; j < 8; ++j)
#pragma unroll
                                for (int f = 0; f < F2; ++f)
                                    acc[f] = mfma4(Wr[((f < HT ? 2 * H + 16 * f : 3 * H + 16 * (f - HT))) * LROW + j], bop[j], acc[f]);
                        }
                    }
                    if (sin >= 0 && has_next) p2(bn, p0, p1);
                    __builtin_amdgcn_sched_barrier(0);
#ifdef PHX_PROF_BLOCKS   // per-block marks: diagnostic build only (run-time branches inside the block loop cost 1-2 %)
                    if (!HOT) tm.mark(14);   // requests + P1'(b) + P2'(b+1)
#endif
                }
            }
            if (sout >= 0) {
                // An owner rewrites a reduced row only after ALL members published the next exchange.  The z_p rows are
                // read by both waves of a pair but produced from the y-waves' partials alone: the y-wave publishes only
                // after its partner has gathered them.
                if (SIDE == 0 && sin >= 0) wait_lds_ge(x, &flag_ag[pr], n_gather);
                u64 *pp = part + (unsigned)((gt * R + (ttl * F4 + SIDE * F2) * 4) * 64);
#pragma unroll
                for (int f = 0; f < F2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st_gran(pp + (unsigned)((f * 4 + r) * 64), lane, acc[f][r], tagOut);
            }
            if (rmode != 0) {
                r0 = sum_over_q(r0); r1 = sum_over_q(r1);
                st_gran(part + (unsigned)((gt * R + RH + 2 * ttl + SIDE) * 64), lane, lq == 0 ? r0 : (lq == 1 ? r1 : 0.f),
                        tagN);
            }
            tm.mark(2);    // partner flag, publishing
        }
        if (SIDE == 0 && sout >= 0) {
            // the a-wave of the pair reads the stage inputs y_s formed here in its next sweep: tell it when they have
            // landed (the drain sits behind the publication, off the critical path of the exchange)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_store(&flag_ys[pr], n_sweep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        tm.mark(sin >= 0 ? 5 : 1);
        // ---- reduce the rows of this exchange that this workgroup owns (this wave: its tiles, its side's sections)
        for (int s = 0; s < nts; ++s) {
            const int ttl = pr * TPW + s;
            if (sout >= 0) {
                const int u0 = (ttl * F4 + SIDE * F2) * 4;
                reduce_owned(u0, u0 + F2 * 4, tagOut, [&](int u) -> unsigned { return (unsigned)(u * 64); },
                             [&](int u, float tot) -> float {
                                 const int r = u & 3, f4 = (u >> 2) % F4, sec = f4 / HT;
                                 const int row = 16 * (f4 % HT) + 4 * lq + r;
                                 if (row >= H) return 0.f;
                                 if (sec == 0) return tot + net.bs[row];          // z_u
                                 if (sec == 1) return expf(tot + net.bp[row]);    // z_p
                                 return tot;                                      // du, dz_p (consumer: dv = dz_p * z_p)
                             });
            }
            if (rmode != 0) {
                const int un = RH + 2 * ttl + SIDE;
                reduce_owned(un, un + 1, tagN,
                             [&](int u) -> unsigned { return (unsigned)((RH + (tagN & 1u) * 2 * ntg + (u - RH)) * 64); },
                             [&](int, float tot) -> float { return tot; });
            }
        }
        tm.mark(3);
    };

    // ---- mixed Linf/RMS norm over the [y, a] blocks (misc.py:14-24) for this wave's controllers; norm rows: lane
    // group lq = slot, lane li = trajectory.  Result per lane (its own trajectory li of tile s): out[s][0..1].
    auto norms = [&](float (&out)[4][2]) {
        const unsigned zn = (unsigned)((RH + (tagN & 1u) * 2 * ntg) * 64);
        if (!shared) {
            for (int s = 0; s < nts; ++s) {
                const int ttl = pr * TPW + s;
                const unsigned offs[2] = {zn + (unsigned)((2 * ttl) * 64), zn + (unsigned)((2 * ttl + 1) * 64)};
                float v[2];
                wait_rows2<2>(x, zb, offs, 2, tagN, lane, v);
                const float y0 = __shfl(v[0], li, 64), a0 = __shfl(v[1], li, 64);
                const float y1 = __shfl(v[0], 16 + li, 64), a1 = __shfl(v[1], 16 + li, 64);
                const double cnt = (double)N;
                out[s][0] = tmaxf(sqrtf((float)((double)y0 / cnt)), sqrtf((float)((double)a0 / cnt)));
                out[s][1] = tmaxf(sqrtf((float)((double)y1 / cnt)), sqrtf((float)((double)a1 / cnt)));
            }
        } else {
            // one controller for the whole batch: sums over every trajectory of every tile, in trajectory order
            double t4[4] = {0.0, 0.0, 0.0, 0.0};
            for (int tl = 0; tl < ntg; ++tl) {
                const unsigned offs[2] = {zn + (unsigned)((2 * tl) * 64), zn + (unsigned)((2 * tl + 1) * 64)};
                float v[2];
                wait_rows2<2>(x, zb, offs, 2, tagN, lane, v);
                for (int k = 0; k < 16; ++k) {
                    if (grp * Bt + tl * 16 + k >= B) break;
                    t4[0] += (double)__shfl(v[0], k, 64); t4[1] += (double)__shfl(v[1], k, 64);
                    t4[2] += (double)__shfl(v[0], 16 + k, 64); t4[3] += (double)__shfl(v[1], 16 + k, 64);
                }
            }
            const double cnt = (double)d.BN;
            const float o0 = tmaxf(sqrtf((float)((double)(float)t4[0] / cnt)), sqrtf((float)((double)(float)t4[1] / cnt)));
            const float o1 = tmaxf(sqrtf((float)((double)(float)t4[2] / cnt)), sqrtf((float)((double)(float)t4[3] / cnt)));
            for (int s = 0; s < nts; ++s) { out[s][0] = o0; out[s][1] = o1; }
        }
        // both waves of the pair have read the reduced norm rows (and finished the sweep before): see "hazards" in DESIGN.md
        pair_sync();
    };

    // -----------------------------------------------------------------------------------------------------------
    // Parameter-gradient quadrature of the stage slots [0, S) with the weights wq (zero => skipped):
    //   a-wave: dWs += (w du)^T a(y_s), dWp += (w dv)^T l(y_s), bias gradients     (A operands: its own hq copies)
    //   y-wave: dWaT += (w z)^T (a_s relu(g)), dg += w a_s (j - y_s) with j - y_s = -sgn k_y / relu(g)
    // Loop order: chunk of QB gene blocks x stage; accumulators stay in registers over the stages of a chunk.
    // First touch of a pair's partial uses plain stores (no memset, no read); later steps read-add-store.
    // -----------------------------------------------------------------------------------------------------------
    bool gfirst = true;
    constexpr int QB = (HT == 3) ? (NP2 == 2 ? 2 : PHX_QB) : 1;
    constexpr int NSEC = (HT == 3) ? 1 : 2;   // HT = 8: the two row sections are accumulated in separate passes
    constexpr int FS = F2 / NSEC;             // hidden tiles per pass
    auto quadrature = [&](auto SC, int S) {
        constexpr int SIDE = decltype(SC)::value;
        tm.mark(0);
        for (int s = 0; s < nts; ++s) {
            const int ttl = pr * TPW + s;
            unsigned actm = 0u;   // stages with a nonzero weight in this tile (wave uniform)
            for (int j = 0; j < S; ++j)
                if (__any(c.wq[(s * 16 + li) * 8 + j] != 0.f)) actm |= 1u << j;
            const bool wr_first = gfirst && s == 0;
            if (actm == 0u && !wr_first) continue;
            const float sgl = c.sgn[s * 16 + li];
            for (int bl0 = 0; bl0 < nbl; bl0 += QB)
            for (int sec = 0; sec < NSEC; ++sec) {
                f32x4 ga[QB][FS][2];
                float dgn[QB][8];
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) dgn[qb][j] = 0.f;
#pragma unroll
                    for (int f = 0; f < FS; ++f)
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) ga[qb][f][s2] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                // Stage pipeline: the raw operands of a stage (transposed hidden rows, state tiles) are turned into MFMA
                // operands, THEN the next active stage's loads are requested, THEN the MFMAs run -- one set of load
                // registers, one memory round trip hidden under 48 QB MFMAs.
                float4 h4raw[FS];
                float xnat[QB][8], knat[QB][8];
                auto issueq = [&](int sidx) {
#pragma unroll
                    for (int f = 0; f < FS; ++f) h4raw[f] = *hqp(s, sidx, sec * FS + f);
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        const int bl = min(bl0 + qb, nbl - 1);
                        // a-wave: a(y_s), l(y_s) from the stage input of y; y-wave: q from the stage input of a
                        load8(tptr(vXS(1 - SIDE, sidx), ttl, bl), xnat[qb]);
                        if (SIDE == 0 && sec == 0) load8(tptr(vK(0, sidx), ttl, bl), knat[qb]);
                    }
                };
                auto next_active = [&](int from) -> int {   // first stage >= from with a nonzero weight in this tile, or S
                    int k = from;
                    while (k < S && !((actm >> k) & 1u)) ++k;
                    return k;
                };
                // quadrature weights of every stage (this lane's own trajectory and the four of its MFMA k-steps) and
                // relu(g) of the chunk's genes: read once, outside the stage loop (LDS round trips off the critical path)
                float wlS[7], w4S[7][4], rrn[QB][8], rrc[QB][2];
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    wlS[k] = c.wq[(s * 16 + li) * 8 + k];
#pragma unroll
                    for (int r = 0; r < 4; ++r) w4S[k][r] = c.wq[(s * 16 + 4 * lq + r) * 8 + k];
                }
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    const float *rg = lds + (long long)min(bl0 + qb, nbl - 1) * BLKF + RGOFF;
#pragma unroll
                    for (int j = 0; j < 8; ++j) rrn[qb][j] = rg[gmap(lq, j)];
                    rrc[qb][0] = rg[gmapC(li, 0)]; rrc[qb][1] = rg[gmapC(li, 1)];
                }
                int sidx = next_active(0);
                // requests are never conditional (a stage past the end re-requests the last one): a conditional request
                // makes the compiler merge register versions with copies that wait for the loads at once
                issueq(min(sidx, S - 1));
                while (sidx < S) {
                    const int snext = next_active(sidx + 1);
                    float wl = 0.f, w4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 7; ++k)
                        if (k == sidx) {
                            wl = wlS[k];
#pragma unroll
                            for (int r = 0; r < 4; ++r) w4[r] = w4S[k][r];
                        }
                    float hd[FS][4], b1[QB][2][4], b2[QB][2][4];
#pragma unroll
                    for (int f = 0; f < FS; ++f) {
                        hd[f][0] = w4[0] * h4raw[f].x; hd[f][1] = w4[1] * h4raw[f].y;
                        hd[f][2] = w4[2] * h4raw[f].z; hd[f][3] = w4[3] * h4raw[f].w;
                    }
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        const int gene0 = (blk0 + min(bl0 + qb, nbl - 1)) * 32;
                        float xr[2][4];
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) xpose4(&xnat[qb][4 * s2], xr[s2], lane);
                        if (SIDE == 0) {
                            if (sec == 0) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) {   // natural layout: this lane's own trajectory
                                    const float rr = rrn[qb][j];
                                    const int gene = gene0 + gmap(lq, j);
                                    const bool ok = rr > 0.f && gene < N && (grp * Bt + ttl * 16 + li) < B;
                                    const float term = wl * (xnat[qb][j] * (-sgl * knat[qb][j] * fast_rcp(rr)));
                                    dgn[qb][j] += ok ? term : 0.f;
                                }
                            }
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) {
                                const bool gok = (gene0 + gmapC(li, s2)) < N;
                                const float rr = rrc[qb][s2];
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const bool ok = gok && (grp * Bt + ttl * 16 + 4 * lq + r) < B;
                                    b1[qb][s2][r] = ok ? xr[s2][r] * rr : 0.f;
                                    b2[qb][s2][r] = b1[qb][s2][r];
                                }
                            }
                        } else {
#pragma unroll
                            for (int s2 = 0; s2 < 2; ++s2) {
                                const bool gok = (gene0 + gmapC(li, s2)) < N;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const bool ok = gok && (grp * Bt + ttl * 16 + 4 * lq + r) < B;
                                    float a, l;
                                    act_pair_fast(xr[s2][r], a, l);
                                    b1[qb][s2][r] = ok ? a : 0.f; b2[qb][s2][r] = ok ? l : 0.f;
                                }
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    issueq(min(snext, S - 1));
                    // rows [0, HT) of the wave's hq are z_u / du (x b1), rows [HT, 2HT) z_p / dv (x b2)
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        if (bl0 + qb >= nbl) continue;
#pragma unroll
                        for (int f = 0; f < FS; ++f) {
                            const bool second = (NSEC == 2) ? (sec == 1) : (f >= HT);
#pragma unroll
                            for (int r = 0; r < 4; ++r)
#pragma unroll
                                for (int s2 = 0; s2 < 2; ++s2)
                                    ga[qb][f][s2] = mfma4(hd[f][r], second ? b2[qb][s2][r] : b1[qb][s2][r], ga[qb][f][s2]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    sidx = snext;
                }
                // ---- store: accumulators are quad-transposed so that a lane owns four consecutive genes of ONE row
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    if (bl0 + qb >= nbl) continue;
                    const int gene0 = (blk0 + bl0 + qb) * 32;
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const int gene4 = gene0 + gmapC(li & ~3, s2), rowq = 4 * lq + (li & 3);
#pragma unroll
                        for (int f = 0; f < FS; ++f) {
                            float a4[4], t0[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) a4[r] = ga[qb][f][s2][r];
                            quad_transpose(a4, t0, lane);
                            const int fg = sec * FS + f;                 // tile within the wave's 2 HT row tiles
                            const int hrow_ = 16 * (fg % HT) + rowq;      // hidden row
                            // y-wave: WaT rows [0,H) (u part) / [H,2H) (p part); a-wave: Ws / Wp
                            const long long base = SIDE == 0 ? oWa + (long long)(fg < HT ? 0 : H) * N
                                                             : (fg < HT ? oWs : oWp);
                            if (hrow_ < H && gene4 < N)
                                add_store4(dth + base + (long long)hrow_ * N + gene4, t0, gene4, N, wr_first);
                        }
                    }
                    if (SIDE == 0 && sec == 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            float dg = dgn[qb][j];
                            dg += __shfl_xor(dg, 1, 64); dg += __shfl_xor(dg, 2, 64);
                            dg += __shfl_xor(dg, 4, 64); dg += __shfl_xor(dg, 8, 64);
                            const int gene = gene0 + gmap(lq, j);
                            if (li == 0 && gene < N) dth[og + gene] = (wr_first ? 0.f : dth[og + gene]) + dg;
                        }
                    }
                }
            }
            // bias gradients: gene independent => only the first gene tile of the group accumulates them
            if (SIDE == 1 && gt == 0) {
#pragma unroll
                for (int f = 0; f < F2; ++f) {
                    float sb = 0.f;
                    for (int sidx = 0; sidx < S; ++sidx) {
                        const float wl = c.wq[(s * 16 + li) * 8 + sidx];
                        if (!__any(wl != 0.f)) continue;
                        const float4 h4 = *hqp(s, sidx, f);
                        sb += c.wq[(s * 16 + 4 * lq + 0) * 8 + sidx] * h4.x + c.wq[(s * 16 + 4 * lq + 1) * 8 + sidx] * h4.y +
                              c.wq[(s * 16 + 4 * lq + 2) * 8 + sidx] * h4.z + c.wq[(s * 16 + 4 * lq + 3) * 8 + sidx] * h4.w;
                    }
                    sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
                    const int hid = 16 * (f % HT) + li;
                    const long long o = (f < HT ? obs : obp) + hid;
                    if (lq == 0 && hid < H) dth[o] = (wr_first ? 0.f : dth[o]) + sb;
                }
            }
        }
        gfirst = false;
        tm.mark(11);
    };

    // -----------------------------------------------------------------------------------------------------------
    // Driver of ONE wave: one call site per building block, sequenced by a phase counter.
    //   dopri5, per interval:  0: f0 input     1: f0, d0, d1 -> h0     2: input y0 + h0 f0     3: f1, d2 -> dt
    //                          4: stage-1 input of a step   5..9: stages 1..5 fused with the next input
    //                          10: stage 6, error ratio -> controller, quadrature, accept pass  (-> 4 while active)
    //   fixed grid:            0: stage-0 input   1..S-1: fused stages   S: last stage -> quadrature, jump
    // -----------------------------------------------------------------------------------------------------------
    const bool dopri = cfg.method == PHX_DOPRI5;
    const bool hot_sweeps = stagger_ticks >= 0;   // diagnostic: a negative stagger selects the generic sweep everywhere
    const int S = dopri ? 7 : fixed_nstages(cfg.method);
    auto any_active = [&]() -> bool {
        bool act = false;
        for (int s = 0; s < nts; ++s) act = act || !c.done[s * 16 + li];
        return __any(act);
    };
    float nv[4][2];
    for (int iv = T - 1; iv >= 1; --iv) {
        if (dopri) {
            for (int s = 0; s < nts; ++s) {
                const int i = s * 16 + li;
                const int b = grp * Bt + (pr * TPW + s) * 16 + li;
                if (lq == 0) {
                    if (b >= B || c.st[i] != PHX_OK) c.done[i] = 1;
                    else {
                        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                        const double sg = (double)c.sgn[i];
                        c.done[i] = 0;
                        c.rk_t0[i] = -sg * tb[iv];
                        c.rk_t1[i] = -sg * tb[iv];
                        c.accept[i] = 0; c.fin[i] = 0;
                        c.nsiv[i] = 0;   // the reference's step budget is per odeint call = per interval (rk_common.py:152-156)
                    }
                }
            }
            wave_lds_sync();
        }
        if (stepped) {
            for (int s = 0; s < nts; ++s) {
                const int i = s * 16 + li;
                const int b = grp * Bt + (pr * TPW + s) * 16 + li;
                if (lq == 0) {
                    if (b >= B || c.st[i] != PHX_OK) c.done[i] = 1;
                    else {
                        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                        const double sg = (double)c.sgn[i];
                        const double u0 = -sg * tb[iv], u1 = -sg * tb[iv - 1];
                        const bool tf32 = cfg.t_is_f32 != 0;
                        const int n = step_grid_steps(u0, u1, cfg.step, tf32);
                        const double g1 = step_grid_at(u0, u1, cfg.step, tf32, n, 1);
                        c.done[i] = 0;
                        if ((long long)n > cfg.max_steps) { c.st[i] = PHX_ERR_MAX_STEPS; c.done[i] = 1; }
                        c.nsiv[i] = 0;
                        c.rk_t0[i] = u0; c.rk_t1[i] = g1;
                        c.dtf[i] = tf32 ? ((float)g1 - (float)u0) : (float)(g1 - u0);
                        c.accept[i] = 0; c.fin[i] = 0;
                    }
                }
            }
            wave_lds_sync();
        }
        int ph = 0;
        bool more = true;
        while (more) {
            int sin = -1, rmode = 0, sout = -1, fmode = F_BASE;
            if (dopri) {
                if (ph == 0) sout = 0;
                else if (ph == 1) { sin = 0; rmode = 1; }
                else if (ph == 2) { sout = 1; fmode = F_H0; }
                else if (ph == 3) { sin = 1; rmode = 2; }
                else if (ph == 4) { sout = 1; fmode = F_DP; }
                else if (ph <= 9) { sin = ph - 4; sout = ph - 3; fmode = F_DP; }
                else { sin = 6; rmode = 3; }
            } else {
                if (ph == 0) sout = 0;
                else if (ph < S) { sin = ph - 1; sout = ph; fmode = F_FIX; }
                else sin = S - 1;
            }
            if (dopri && ph >= 5 && ph <= 9 && hot_sweeps) {   // the five fused stages of a dopri5 step: compile-time shapes
                const int hs = ph - 4;
                if (side == 0) {
                    if (hs == 1) sweep(IC<0>{}, IC<1>{}, 0, 0, 0, 0, iv);
                    else if (hs == 2) sweep(IC<0>{}, IC<2>{}, 0, 0, 0, 0, iv);
                    else if (hs == 3) sweep(IC<0>{}, IC<3>{}, 0, 0, 0, 0, iv);
                    else if (hs == 4) sweep(IC<0>{}, IC<4>{}, 0, 0, 0, 0, iv);
                    else sweep(IC<0>{}, IC<5>{}, 0, 0, 0, 0, iv);
                } else {
                    if (hs == 1) sweep(IC<1>{}, IC<1>{}, 0, 0, 0, 0, iv);
                    else if (hs == 2) sweep(IC<1>{}, IC<2>{}, 0, 0, 0, 0, iv);
                    else if (hs == 3) sweep(IC<1>{}, IC<3>{}, 0, 0, 0, 0, iv);
                    else if (hs == 4) sweep(IC<1>{}, IC<4>{}, 0, 0, 0, 0, iv);
                    else sweep(IC<1>{}, IC<5>{}, 0, 0, 0, 0, iv);
                }
            } else if (side == 0) sweep(IC<0>{}, IC<0>{}, sin, rmode, sout, fmode, iv);
            else sweep(IC<1>{}, IC<0>{}, sin, rmode, sout, fmode, iv);
            if (rmode != 0) {
                norms(nv);
                tm.mark(8);
            }
            if (!dopri) {
                if (ph < S) { ++ph; continue; }
                // ---- end of the reversed fixed-grid step: quadrature weights = the step's combination weights
                pair_sync();   // the partner's stage tiles are complete (no norm exchange orders them here)
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    const int b = grp * Bt + (pr * TPW + s) * 16 + li;
                    const bool act = !c.done[i];
                    const float dtl = dt_rev(i, b, iv);
                    if (lq == 0) {
                        for (int j = 0; j < 8; ++j)
                            c.wq[i * 8 + j] = (act && j < S) ? c.sgn[i] * fixed_weight(cfg.method, j, dtl) : 0.f;
                        if (act) {   // (sub-steps: the interval ends, and the jump happens, with the last step of its grid)
                            c.nsteps[i] += 1; c.nfe[i] += S; c.accept[i] = 1;
                            int fin = 1;
                            if (stepped) {
                                const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                                const double sg = (double)c.sgn[i];
                                fin = c.nsiv[i] + 1 >= step_grid_steps(-sg * tb[iv], -sg * tb[iv - 1], cfg.step, cfg.t_is_f32 != 0);
                            }
                            c.fin[i] = fin;
                        }
                    }
                }
                wave_lds_sync();
            } else if (ph == 1) {
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    if (lq == 0 && !c.done[i]) {
                        c.h0f[i] = init_h0(nv[s][0], nv[s][1]);
                        c.d1[i] = nv[s][1];
                    }
                }
                wave_lds_sync();
                ++ph;
                continue;
            } else if (ph == 3) {
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    if (lq == 0 && !c.done[i]) {
                        const float h0 = c.h0f[i];
                        const float d2 = nv[s][0] / h0;
                        const double dt = init_dt(h0, c.d1[i], d2);
                        c.dt[i] = dt; c.dtf[i] = (float)dt; c.nfe[i] += 2;
                        const double t0 = c.rk_t1[i];
                        if (!(t0 + dt > t0)) { c.st[i] = PHX_ERR_DT_UNDERFLOW; c.done[i] = 1; }
                    }
                }
                wave_lds_sync();
                more = any_active() && !x.aborted;
                ++ph;
                continue;
            } else if (ph < 10) {
                ++ph;
                continue;
            } else {
                // ---- controller (rk_common.py:150-220)
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    const int b = grp * Bt + (pr * TPW + s) * 16 + li;
                    if (lq == 0 && !c.done[i]) {
                        const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                        const double sg = (double)c.sgn[i];
                        const double u_end = -sg * tb[iv - 1];
                        const float ratio = nv[s][0];
                        const int acc = (ratio <= 1.0f) ? 1 : 0;
                        const double t0 = c.rk_t1[i], dt = c.dt[i];
                        const double t1 = t0 + dt;
                        c.rk_t0[i] = t0;
                        c.rk_t1[i] = acc ? t1 : t0;
                        c.accept[i] = acc;
                        c.nsteps[i] += 1;
                        const int ns = c.nsiv[i] + 1;
                        c.nsiv[i] = ns;
                        c.nfe[i] += 6;
                        const float dtf = c.dtf[i];
                        c.dtp[i] = dtf;
                        int fin = 0;
                        double xx = 1.0;
                        if (acc && u_end <= t1) { fin = 1; xx = (u_end - t0) / (t1 - t0); }
                        c.xfin[i] = xx;
                        for (int j = 0; j < 8; ++j) {
                            float wj = 0.f;
                            if (acc && j < 7) {
                                double W;
                                if (!fin) W = DP_CSOL64[j];
                                else {
                                    const double x2 = xx * xx, x3 = x2 * xx, x4 = x3 * xx;
                                    const double d1 = (j == 0) ? 1.0 : 0.0, d7 = (j == 6) ? 1.0 : 0.0;
                                    const double cj = DP_CSOL64[j], mj = DP_CMID64[j];
                                    W = xx * d1 + x2 * (d7 - 4.0 * d1 - 5.0 * cj + 16.0 * mj) +
                                        x3 * (5.0 * d1 - 3.0 * d7 + 14.0 * cj - 32.0 * mj) +
                                        x4 * (2.0 * d7 - 2.0 * d1 - 8.0 * cj + 16.0 * mj);
                                }
                                wj = (float)(sg * (double)dtf * W);
                            }
                            c.wq[i * 8 + j] = wj;
                        }
                        const double dtn = optimal_step_size(dt, ratio);
                        c.dt[i] = dtn; c.dtf[i] = (float)dtn;
                        int dn = fin;
                        if (!dn) {   // the reference tests the step budget first, then the step size (rk_common.py:154,175)
                            const double tn = c.rk_t1[i];
                            if ((long long)ns >= cfg.max_steps) { c.st[i] = PHX_ERR_MAX_STEPS; dn = 2; }
                            else if (!(tn + dtn > tn)) { c.st[i] = PHX_ERR_DT_UNDERFLOW; dn = 2; }
                        }
                        c.fin[i] = dn;   // 0: continue, 1: reached t_{i-1}, 2: failed
                    }
                }
                wave_lds_sync();
                tm.mark(9);
            }
            if (want_grads) {
                if (side == 0) quadrature(IC<0>{}, S);
                else quadrature(IC<1>{}, S);
            }
            // both waves are done reading each other's stage tiles: the accept pass and the next step may overwrite them
            pair_sync();
            // ---- accept pass.  dopri5: advance the state (dense output of the adjoint at the interval end), FSAL copies
            // of stage slot 6.  Fixed grid: every active trajectory "finishes" its interval with the step's combination.
            // Either way the interval ends with the jump  aug_state[1] = y[i-1]; aug_state[2] += grad_y[i-1]
            // (adjoint.py:152-154).
            for (int s = 0; s < nts; ++s) {
                const int ttl = pr * TPW + s;
                const int i = s * 16 + li;
                const int b = grp * Bt + ttl * 16 + li;
                const bool adv = !c.done[i] && c.accept[i];
                const int fin = c.fin[i];
                if (!__any(adv)) continue;
                const bool anyfin = __any(adv && fin == 1), anyfsal = dopri && __any(adv && fin != 1);
                const float dts = dopri ? c.dtp[i] : dt_rev(i, b, iv);
                const InterpX ix = make_interp_x(c.xfin[i]);
                for (int bl = 0; bl < nbl; ++bl) {
                    float x1[8], k6[8], xnew[8], jump[8];
                    if (dopri) {
                        load8(tptr(vXS(side, 6), ttl, bl), x1);
                        load8(tptr(vK(side, 6), ttl, bl), k6);
                    } else if (side == 1 || __any(adv && fin != 1)) {
                        // the step's own combination (fixed_grid.py, rk_common.py:96-103); the y-wave needs it only for a
                        // sub-step inside an interval: at the interval's end its state is replaced by the saved one
                        float a0[8], f0[8], kq[3][8];
                        load8(tptr(vX0(side), ttl, bl), a0);
                        load8(tptr(vK(side, 0), ttl, bl), f0);
                        if (S >= 2) load8(tptr(vK(side, 1), ttl, bl), kq[0]);
                        if (S >= 4) { load8(tptr(vK(side, 2), ttl, bl), kq[1]); load8(tptr(vK(side, 3), ttl, bl), kq[2]); }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if (cfg.method == PHX_EULER) x1[j] = a0[j] + dts * f0[j];
                            else if (cfg.method == PHX_MIDPOINT) x1[j] = a0[j] + dts * kq[0][j];
                            else x1[j] = a0[j] + (((f0[j] + 3.0f * (kq[0][j] + kq[1][j])) + kq[2][j]) * dts) * 0.125f;
                        }
                    }
                    {   // jump data of the trajectories that reach t_{i-1} in this step
                        const long long ro = (long long)(iv - 1) * d.BN + (long long)b * N;
                        const int g0 = (blk0 + bl) * 32 + gmap(lq, 0);
                        row_load8(side ? grad_y : y_saved, ro, g0, N, (b < B) && fin == 1, side ? 0.f : 0.5f, jump);
                    }
                    if (side == 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) xnew[j] = (fin == 1) ? jump[j] : x1[j];
                    } else {
                        float aout[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) aout[j] = x1[j];
                        if (anyfin && dopri) {   // quartic dense output of the adjoint at u_end (interp.py)
                            float a0[8], f0[8], kq[4][8];
                            load8(tptr(vX0(1), ttl, bl), a0);
                            load8(tptr(vK(1, 0), ttl, bl), f0);
                            {
                                float am[8];
#pragma unroll
                                for (int kk = 0; kk < 4; ++kk) load8(tptr(vK(1, 2 + kk), ttl, bl), kq[kk]);   // c_mid2 = 0
#pragma unroll
                                for (int j = 0; j < 8; ++j) am[j] = f0[j] * (dts * DP_CMID[0]);
#pragma unroll
                                for (int kk = 0; kk < 4; ++kk) {
                                    const float cf = dts * DP_CMID[2 + kk];
#pragma unroll
                                    for (int j = 0; j < 8; ++j) am[j] += kq[kk][j] * cf;
                                }
#pragma unroll
                                for (int j = 0; j < 8; ++j) {
                                    am[j] += k6[j] * (dts * DP_CMID[6]);
                                    aout[j] = interp_eval(a0[j], x1[j], a0[j] + am[j], f0[j], k6[j], dts, ix);
                                }
                            }
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) xnew[j] = (fin == 1) ? aout[j] + jump[j] : x1[j];
                    }
                    if (adv) {
                        store8(tptr(vX0(side), ttl, bl), xnew);
                        if (dopri && fin != 1) {   // FSAL: stage-7 data is stage-1 data of the next step
                            store8(tptr(vK(side, 0), ttl, bl), k6);
                            store8(tptr(vXS(side, 0), ttl, bl), x1);
                        }
                    }
                }
                if (want_grads && anyfsal) {   // the transposed hidden rows follow: register r <-> trajectory 4 lq + r
#pragma unroll
                    for (int f = 0; f < F2; ++f) {
                        const float4 h6 = *hqp(s, 6, f);
                        float4 h0 = *hqp(s, 0, f);
                        const int l4 = s * 16 + 4 * lq;
                        if (!c.done[l4 + 0] && c.accept[l4 + 0] && c.fin[l4 + 0] != 1) h0.x = h6.x;
                        if (!c.done[l4 + 1] && c.accept[l4 + 1] && c.fin[l4 + 1] != 1) h0.y = h6.y;
                        if (!c.done[l4 + 2] && c.accept[l4 + 2] && c.fin[l4 + 2] != 1) h0.z = h6.z;
                        if (!c.done[l4 + 3] && c.accept[l4 + 3] && c.fin[l4 + 3] != 1) h0.w = h6.w;
                        *hqp(s, 0, f) = h0;
                    }
                }
            }
            wave_lds_sync();   // the hq copy above read accept/fin of other lanes before they are reset below
            tm.mark(10);
            if (stepped) {
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    const int b = grp * Bt + (pr * TPW + s) * 16 + li;
                    if (lq == 0) {
                        if (!c.done[i] && c.fin[i]) {
                            c.done[i] = 1;
                            for (int j = 0; j < 8; ++j) c.wq[i * 8 + j] = 0.f;
                        } else if (!c.done[i]) {   // next step of this interval's grid
                            const TimeRow tb = trowT(t, T, cfg, shared ? 0 : b);
                            const double sg = (double)c.sgn[i];
                            const bool tf32 = cfg.t_is_f32 != 0;
                            const int k = c.nsiv[i] + 1;
                            const double g0 = c.rk_t1[i];
                            const double u0 = -sg * tb[iv], u1 = -sg * tb[iv - 1];
                            const double g1 = step_grid_at(u0, u1, cfg.step, tf32, step_grid_steps(u0, u1, cfg.step, tf32), k + 1);
                            c.nsiv[i] = k;
                            c.rk_t0[i] = g0; c.rk_t1[i] = g1;
                            c.dtf[i] = tf32 ? ((float)g1 - (float)g0) : (float)(g1 - g0);
                        }
                        c.accept[i] = 0; c.fin[i] = 0;
                    }
                }
                wave_lds_sync();
                more = any_active() && !x.aborted;
                ph = 0;
            } else if (!dopri) {
                for (int s = 0; s < nts; ++s)
                    if (lq == 0) { c.accept[s * 16 + li] = 0; c.fin[s * 16 + li] = 0; }
                wave_lds_sync();
                more = false;
            } else {
                for (int s = 0; s < nts; ++s) {
                    const int i = s * 16 + li;
                    if (lq == 0 && !c.done[i] && c.fin[i]) {
                        c.done[i] = 1;
                        for (int j = 0; j < 8; ++j) c.wq[i * 8 + j] = 0.f;
                    }
                }
                wave_lds_sync();
                more = any_active() && !x.aborted;
                ph = 4;
            }
        }
    }

    // ---- results
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (side == 1)
        for (int s = 0; s < nts; ++s) {
            const int ttl = pr * TPW + s;
            const int b = grp * Bt + ttl * 16 + li;
            for (int bl = 0; bl < nbl; ++bl) {
                float a0[8];
                load8(tptr(vX0(1), ttl, bl), a0);
                row_store8(adj_y0, (long long)b * N, (blk0 + bl) * 32 + gmap(lq, 0), N, b < B, a0);
            }
        }
    tm.mark(0);
    if (tm.on) tacc[15] = (unsigned long long)clock64() - tacc[15];
    if (tm.on)
        for (int k = 0; k < 16; ++k) w.prof[(long long)blockIdx.x * 16 + k] = tm.acc[k];
    if (gt == 0 && side == 0)
        for (int s = 0; s < nts; ++s) {
            const int i = s * 16 + li;
            const int b = grp * Bt + (pr * TPW + s) * 16 + li;
            if (lq == 0 && b < B) {
                status[b] = x.aborted ? (int)PHX_ERR_SYNC_TIMEOUT : c.st[i];
                nfe_out[b] = c.nfe[i];
                nsteps_out[b] = c.nsteps[i];
            }
        }
}

}  // namespace
