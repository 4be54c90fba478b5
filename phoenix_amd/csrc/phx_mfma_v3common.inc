// phx_mfma_v3common.inc -- helpers shared by the third-generation solve kernels (k1_solve_adj3, k1_solve_fwd3):
// buffer-resource addressing of the private tiles, write-through / volatile forms for rows other workgroups read, the
// out-of-line controller math.  Included inside each translation unit after phx_mfma_common.inc.
namespace {

template <int V>
struct I3 { static constexpr int value = V; };

// Hidden-row order inside a 16-row tile of the third-generation kernels.  The MFMA M / K index m = 4 q + r (q: lane
// group, r: accumulator register or k-step) stands for tile row rho16(q, r): k-steps (registers) 0, 1 hold rows 0..7,
// k-steps 2, 3 rows 8..15.  A last tile with only 8 live rows (H = 40: rows 40..47 are padding) then costs TWO k-steps of
// every product that contracts over hidden rows and ONE granule pair per section in the exchange instead of four / two
// (the natural order 4 q + r spreads the padding rows over all k-steps).  Inside a k-step the four rows sit at offsets
// {0, 4, 1, 5}: rows = 0 and = 4 (mod 8) pair up, so with LROW = 33 the LDS reads of both operand forms touch every bank
// exactly twice per wave, like the natural order did.  HALF (template flag of the kernels) = the last tile is such a tile.
__host__ __device__ constexpr int rho16(int q, int r) { return 8 * (r >> 1) + 2 * (r & 1) + 4 * (q & 1) + (q >> 1); }

// The held genes of one call (the CLAMP forms of k1_solve_fwd3 / k1_solve_fwd3c): row `grp` of the [calls, width] list,
// read once per workgroup into wave-uniform values.  Slots beyond the width are -1, which like every index that no gene
// has (padding of a shorter set) matches nothing.
struct ClampSet {
    int g[PHX_CLAMP_MAX];
};
__device__ __forceinline__ ClampSet clamp_set(const int *__restrict__ list, int grp, int width)
{
    ClampSet s;
#pragma unroll
    for (int i = 0; i < PHX_CLAMP_MAX; ++i)
        s.g[i] = i < width ? __builtin_amdgcn_readfirstlane(list[(long long)grp * width + i]) : -1;
    return s;
}
// The held genes of one trajectory ROW (the CLAMP forms without CALLS, and k1_solve_adj3's): row `b` of the [B, width]
// list, one set per lane (the lane's trajectory), in vector registers.  A padding row (b >= B) reads nothing and holds
// nothing.
__device__ __forceinline__ ClampSet clamp_set_row(const int *__restrict__ list, int b, int B, int width)
{
    ClampSet s;
#pragma unroll
    for (int i = 0; i < PHX_CLAMP_MAX; ++i) s.g[i] = (i < width && b < B) ? list[(long long)b * width + i] : -1;
    return s;
}
__device__ __forceinline__ bool clamp_holds(const ClampSet &s, int gene)
{
    bool hit = false;
#pragma unroll
    for (int i = 0; i < PHX_CLAMP_MAX; ++i) hit |= gene == s.g[i];
    return hit;
}

// Two sets of exchange buffers per workspace, used alternately (no fill between launches).  The exchange protocol needs
// every granule of a launch to start with a tag that is not one of the launch's own (tags restart at 1).  Instead of a
// 12-24 MB fill in front of every launch, a launch works in set S = parity of its batch group (a header word in the
// workspace) and zero-fills the OTHER set for its successor while it starts up: each workgroup clears its own member
// region of the partial rows and its share of the reduced rows (plain stores; nobody reads that set during this launch;
// the kernel boundary makes them visible).  The group leader flips the parity at the very end -- after every workgroup
// of the group has announced that it has read it (`started` counter), so that a group without any exchange (T < 2, all
// trajectories done) cannot flip it under a late starter.  Header words (unsigned int, in W1::cnt; TG <= 256): [grp] parity,
// [256 + s] abort flag of set s, [512 + grp] started counter.  The library fills header + set 0 whenever the caller does
// not vouch for the workspace (phx_solve_opts.ws_keep = 0) or walks a batch in chunks: parity 0, set 0 clean, set 1 is
// cleaned by that launch itself.
struct XSet {
    unsigned int *hdr;
    unsigned int s;   // the set this launch works in
};
__device__ __forceinline__ XSet xset_begin(const W1 &w, int grp, int gt, int G, int R, unsigned long long *&part,
                                           unsigned long long *&zbuf, unsigned int *&abort_flag)
{
    unsigned int *hdr = reinterpret_cast<unsigned int *>(w.cnt);
    const unsigned int s = (unsigned int)__builtin_amdgcn_readfirstlane(
                               (int)__hip_atomic_load(&hdr[grp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 1u;
    __syncthreads();   // every thread of the workgroup has the parity before the workgroup announces itself
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&hdr[512 + grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long *const p_use = s ? w.part1 : w.part, *const z_use = s ? w.zbuf1 : w.zbuf;
    unsigned long long *const p_clr = s ? w.part : w.part1, *const z_clr = s ? w.zbuf : w.zbuf1;
    part = p_use + (long long)grp * G * R * 64;
    zbuf = z_use + (long long)grp * R * 64;
    abort_flag = &hdr[256 + s];
    // clean the other set for the next launch: this member's partial rows (R rows of 64 granules), its share of the group's
    // reduced rows, and the other set's abort flag
    ulonglong2 *pz = reinterpret_cast<ulonglong2 *>(p_clr + ((long long)grp * G + gt) * R * 64);
    for (int i = threadIdx.x; i < R * 32; i += blockDim.x) pz[i] = make_ulonglong2(0ull, 0ull);
    for (int r = gt; r < R; r += G) {
        ulonglong2 *zz = reinterpret_cast<ulonglong2 *>(z_clr + ((long long)grp * R + r) * 64);
        if (threadIdx.x < 32) zz[threadIdx.x] = make_ulonglong2(0ull, 0ull);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[256 + (1u - s)] = 0u;
    return XSet{hdr, s};
}
// very end of the kernel: the group leader waits until all G workgroups of the group have read the parity, then flips it
__device__ __forceinline__ void xset_end(const XSet &xs, int grp, int gt, int G)
{
    if (gt == 0 && threadIdx.x == 0) {
        unsigned long long t0 = 0;
        unsigned int spins = 0;
        while (__hip_atomic_load(&xs.hdr[512 + grp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)G) {
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 255u) == 0) {
                if (t0 == 0) t0 = wall_clock64();
                if (wall_clock64() - t0 > 500000000ull) break;   // 5 s: the launch was not fully resident
            }
        }
        __hip_atomic_store(&xs.hdr[512 + grp], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&xs.hdr[grp], xs.s ^ 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Hand-over of k1_solve_adj3's last quadrature + accept visit to the tail kernel (k3_tail_adj3, phx_mfma_adj3_tail.inc).
// A batch group that defers the visit writes, into the head of its own (otherwise unwritten) gradient partial, one record
// of TR_N floats per trajectory -- the seven stage weights, the step, the direction, the powers of the dense-output
// fraction, 1.0 where the trajectory advances -- and behind the Bt records the ring base of every trajectory tile; header
// word XH_DEFER + grp of the workspace says whether the group deferred in this launch (written by every launch that
// wants gradients: the partial itself cannot say, any bit pattern may be a gradient).  XH_SERVED: the number of deferred
// groups the last tail launch worked on (diagnostic; phx_debug_adj3_tail_words).
enum { C_Y0 = 0, C_A0 = 1, C_KY = 2, C_KA = 9 };   // k1_solve_adj3's private vectors: Y0, A0, KY[7], KA[7]
enum { TR_W = 0, TR_DT = 7, TR_SG = 8, TR_X = 9, TR_ADV = 13, TR_N = 16 };
constexpr int XH_DEFER = 768, XH_SERVED = 300;   // (header words: [0, 256) parity, 256 / 257 abort flags, [512, 768) started)
__host__ __device__ inline size_t tail_record_floats(int Bt, int ntg) { return (size_t)Bt * TR_N + (size_t)ntg; }

// Private tiles and the transposed hidden rows are addressed through buffer resources: the address of an access is
// (resource in SGPRs) + (scalar offset of the tile, computed by the scalar unit) + (ONE 32-bit lane offset shared by all
// accesses) + immediate.  With flat 64-bit pointers the compiler keeps a per-lane 64-bit address per live tile pointer
// (two vector registers each, vector adds to advance them) and spills them.
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ void bload4(__amdgpu_buffer_rsrc_t r, int voff, int soff, float *x)
{
    const i32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    x[0] = __int_as_float(u.x); x[1] = __int_as_float(u.y); x[2] = __int_as_float(u.z); x[3] = __int_as_float(u.w);
}
__device__ __forceinline__ void bload8(__amdgpu_buffer_rsrc_t r, int voff, int soff, float *x)
{
    bload4(r, voff, soff, x);
    bload4(r, voff + 16, soff, x + 4);
}
// HARDWARE HAZARD, not covered by the compiler (found in round 4; reproducer: tools/membench/store_war.hip).  On gfx950 a
// VALU instruction that overwrites the data VGPRs of a 128-bit buffer store within the next wait state changes what the
// store writes for lanes 12..15 of every 16 (the store fetches that part of its data late).  LLVM's hazard recognizer
// knows the hazard ("VALU writes the data of a VMEM store wider than 64 bits": 2 wait states on gfx940+) but exempts
// MUBUF stores whose soffset is an SGPR (GCNHazardRecognizer::createsVALUHazard) -- exactly the form every access of
// these kernels has (buffer resource + scalar tile / row offset + one lane offset).  Whether a build was hit depended on
// register allocation alone: the store's data tuple had to be re-used by the very next instruction.  That is the
// "trajectories 12..15 of a tile take thousands of steps" signature of DESIGN.md section 2 (lanes 12..15 + 16 q of a
// tile = trajectories 12..15: their FSAL slope k_7 tile held values of ANOTHER vector).
// bstore_guard keeps the tuple alive across two wait states behind its store: the `s_nop 1` reads the tuple (so the
// register allocator cannot hand its registers out earlier) and is ordered behind the store by its memory clobber.
// EVERY 128-bit buffer store of the third-generation kernels goes through store128 below.
__device__ __forceinline__ void bstore_guard(const i32x4 &u) { asm volatile("s_nop 1" ::"v"(u) : "memory"); }
template <int AUX>
__device__ __forceinline__ void store128(const i32x4 &u, __amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b128(u, r, voff, soff, AUX);
    bstore_guard(u);
}
__device__ __forceinline__ void bstore4(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float *x)
{
    const i32x4 u = {__float_as_int(x[0]), __float_as_int(x[1]), __float_as_int(x[2]), __float_as_int(x[3])};
    store128<0>(u, r, voff, soff);
}
// write-through / L1-bypassing forms (sc1) for rows that other workgroups read (MI355X_MICROARCH.md, valid hand-off forms)
__device__ __forceinline__ void bstore4_sc1(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float *x)
{
    const i32x4 u = {__float_as_int(x[0]), __float_as_int(x[1]), __float_as_int(x[2]), __float_as_int(x[3])};
    store128<16>(u, r, voff, soff);
}
__device__ __forceinline__ void bload4_sc1(__amdgpu_buffer_rsrc_t r, int voff, int soff, float *x)
{
    const i32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, (int)0x80000010);   // + volatile
    x[0] = __int_as_float(u.x); x[1] = __int_as_float(u.y); x[2] = __int_as_float(u.z); x[3] = __int_as_float(u.w);
}
__device__ __forceinline__ void bstore8(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float *x)
{
    bstore4(r, voff, soff, x);
    bstore4(r, voff + 16, soff, x + 4);
}

__device__ __forceinline__ void act_grad_fast3(float y, float &da, float &dl)
{
    const float s = y - 0.5f;
    const float d = 1.0f + fabsf(s);
    const float rd = fast_rcp(d);
    da = rd * rd;
    dl = (s < 0.0f) ? rd : fast_rcp((1.0f + s) * (1.0f + 2.0f * s));
}

// The controller's libm calls (pow in fp64 / fp32) are kept out of line: inlined, their coefficient tables are hoisted
// out of the persistent step loop and occupy (spilled) registers for the whole kernel.
__device__ __noinline__ double optimal_step_size_ni(double last_step, float error_ratio)
{
    return optimal_step_size(last_step, error_ratio);
}
__device__ __noinline__ double init_dt_ni(float h0, float d1, float d2) { return init_dt(h0, d1, d2); }


// One chunk of `nbl` gene blocks, all blocks' loads in flight at once (the per-block form of stage_images is one exposed
// round trip per block).  Images of consecutive blocks of one chunk are BF * HC floats apart.
template <int NF>
__device__ __forceinline__ void stage_chunk_flat(const float *__restrict__ wimg, float *lds, int blk0, int nbl, int ch, int HC,
                                                 int BF)
{
    // (block, element) of a thread's successive float4s advance without divisions: a block image (> 1 300 float4) is longer
    // than the workgroup's stride (256 threads)
    const int per = BF >> 2, nth = (int)blockDim.x;
    int bl = 0, e = threadIdx.x;
    while (bl < nbl) {
        float4 v[NF];
        int dst[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const int blc = min(bl, nbl - 1);
            dst[k] = bl < nbl ? bl * per + e : -1;
            v[k] = reinterpret_cast<const float4 *>(wimg + ((long long)(blk0 + blc) * HC + ch) * BF)[e];
            e += nth;
            if (e >= per) { e -= per; ++bl; }
        }
#pragma unroll
        for (int k = 0; k < NF; ++k)
            if (dst[k] >= 0) reinterpret_cast<float4 *>(lds)[dst[k]] = v[k];
    }
}


// The same walk split in two, for a chunk that is requested while the current one is still computing: chunk_issue puts the
// loads in flight (NF float4 per thread, enough for gene tiles of up to four blocks: 24 x 256 threads >= 4 x 1 394), the values
// wait in registers under the MFMA phases, chunk_commit writes them to the slot between the two barriers of the switch.
typedef float v4f __attribute__((ext_vector_type(4)));   // (a plain vector type: arrays of HIP's float4 struct were left in scratch)
template <int NF>
__device__ __forceinline__ void chunk_issue(const float *__restrict__ wimg, int blk0, int nbl, int ch, int HC, int BF,
                                            v4f (&v)[NF])
{
    const int per = BF >> 2, nth = (int)blockDim.x;
    int bl = 0, e = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const int blc = min(bl, nbl - 1);
        v[k] = reinterpret_cast<const v4f *>(wimg + ((long long)(blk0 + blc) * HC + ch) * BF)[e];
        e += nth;
        if (e >= per) { e -= per; ++bl; }
    }
}
template <int NF>
__device__ __forceinline__ void chunk_commit(float *lds, int nbl, int BF, const v4f (&v)[NF])
{
    const int per = BF >> 2, nth = (int)blockDim.x;
    int bl = 0, e = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        if (bl < nbl) reinterpret_cast<v4f *>(lds)[bl * per + e] = v[k];
        e += nth;
        if (e >= per) { e -= per; ++bl; }
    }
}


// Small batches: one batch group whose trajectory tiles leave at least half of the workgroup's waves without a tile (the
// reference's own batch sizes: 17 at the breast-cancer shape = 2 tiles on 4 waves).  Instead of idling as exchange helpers
// the waves of a tile SPLIT ITS GENE BLOCKS: wave w works on tile w mod ntg, block part w / ntg of `nparts` = NW / ntg; the
// partial hidden rows (and norm partials) of a tile's waves are added in LDS -- in part order, deterministic -- before part 0
// publishes them.  Measured before (round 5, B = 17 / 32 at C4): the sweeps were a third of both launches and ran on two of
// four SIMDs.
__host__ __device__ inline int v3_split_parts(int TG, int NW, int TPW, int ntg)
{
    return (TG == 1 && TPW == 1 && ntg >= 1 && ntg * 2 <= NW) ? NW / ntg : 1;
}
// LDS of the combine: [wave][rows + 1 (norm partials)][64 lanes] float4
__host__ __device__ inline size_t v3_comb_bytes(int NW, int rows) { return (size_t)NW * (rows + 1) * 1024; }


// Tile-slot accesses of GW = 8 (a whole gene block per workgroup) or 4 floats per lane (HALF-BLOCK gene tiles of the chunked
// kernels: the workgroup owns 16 genes, the second 16 bytes of a lane's slot belong to its sibling), and the caller's rows
template <int GW>
__device__ __forceinline__ void tload(__amdgpu_buffer_rsrc_t r, int voff, int soff, float *x)
{
    bload4(r, voff, soff, x);
    if (GW == 8) bload4(r, voff + 16, soff, x + 4);
}
template <int GW>
__device__ __forceinline__ void tstore(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float *x)
{
    bstore4(r, voff, soff, x);
    if (GW == 8) bstore4(r, voff + 16, soff, x + 4);
}
__device__ __forceinline__ void row_load4(const float *__restrict__ a, long long rowoff, int g0, int N, bool rowok, float fill, float *x)
{
    if (rowok && g0 + 4 <= N) {
        const F4A u = *reinterpret_cast<const F4A *>(a + rowoff + g0);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = u.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = (rowok && g0 + j < N) ? a[rowoff + g0 + j] : fill;
    }
}
__device__ __forceinline__ void row_store4(float *__restrict__ a, long long rowoff, int g0, int N, bool rowok, const float *x)
{
    if (!rowok) return;
    if (g0 + 4 <= N) {
        F4A u;
#pragma unroll
        for (int j = 0; j < 4; ++j) u.v[j] = x[j];
        *reinterpret_cast<F4A *>(a + rowoff + g0) = u;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g0 + j < N) a[rowoff + g0 + j] = x[j];
    }
}
template <int GW>
__device__ __forceinline__ void row_loadG(const float *__restrict__ a, long long rowoff, int g0, int N, bool rowok, float fill, float *x)
{
    if (GW == 8) row_load8(a, rowoff, g0, N, rowok, fill, x);
    else row_load4(a, rowoff, g0, N, rowok, fill, x);
}
template <int GW>
__device__ __forceinline__ void row_storeG(float *__restrict__ a, long long rowoff, int g0, int N, bool rowok, const float *x)
{
    if (GW == 8) row_store8(a, rowoff, g0, N, rowok, x);
    else row_store4(a, rowoff, g0, N, rowok, x);
}


// MFMA chains whose A operands come from LDS, one read per MFMA: left to itself the compiler issues an operand's read one or
// two MFMAs ahead of its use (it minimises registers), and every group of MFMAs waits out most of the LDS latency -- the
// clusters ran at 45-55 % of their MFMA time.  mfma_steps pins the software pipeline: the reads of step s + D are issued
// before the MFMAs of step s (scheduling barriers: nothing moves across), D + 1 register sets of K operands.  The order of
// the MFMAs -- every accumulation chain -- is the caller's: results are bitwise what the plain loop gives.
//   load(s, w): read the K operands of step s into w[0..K);   mma(s, w): the step's MFMAs
template <int NS, int D, int K, class LoadF, class MmaF>
__device__ __forceinline__ void mfma_steps(LoadF &&load, MmaF &&mma)
{
    float wb[D + 1][K];
#pragma unroll
    for (int s = 0; s < D && s < NS; ++s) load(s, wb[s % (D + 1)]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + D < NS) load(s + D, wb[(s + D) % (D + 1)]);
        __builtin_amdgcn_sched_barrier(0);
        mma(s, wb[s % (D + 1)]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace
