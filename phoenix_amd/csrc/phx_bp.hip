// phx_bp.hip -- translation unit of the fixed-grid backpropagation kernel (k1_solve_bp, phx_mfma_bp.inc): launch
// planning, workspace layout and the host entry points the C ABI (phx_engine.hip) calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "phx_solver.hpp"
#include "phx_host.hpp"

using namespace phxh;

#include "phx_mfma_common.inc"
#include "phx_mfma_adj2.inc"   // the bounded polls (wait_members), act_grad_fast2, IC<>
#include "phx_mfma_bp.inc"

namespace {

constexpr size_t BP_LDS_TAIL = 256;

// Four waves per workgroup, one trajectory tile each; the smallest NB (gene blocks per workgroup) whose grid the device
// holds at once.  H <= 128: the weight images of a gene block stay LDS resident, like k1_solve_adj2.
bool plan_bp_cus(int cus, int N, int H, int B, int T, D1 *out)
{
    if (cus <= 0 || N <= 0 || H <= 0 || H > 128 || B <= 0 || force_v0()) return false;
    const int HT = H <= 48 ? 3 : 8;
    const size_t blkbytes = (size_t)blk_floats_ch(HT, H) * 4;
    if (blkbytes + BP_LDS_TAIL > LDS_BUDGET) return false;
    const int nblk = (N + 31) / 32, ntt = (B + 15) / 16;
    const int TG = (ntt + BP_NW - 1) / BP_NW;
    const int ntg = TG == 1 ? ntt : BP_NW;
    const int NBmax = (int)std::min<size_t>((LDS_BUDGET - BP_LDS_TAIL) / blkbytes, 8);
    for (int NB = 1; NB <= NBmax; ++NB) {
        const int G = (nblk + NB - 1) / NB;
        if ((long long)TG * G > cus) continue;
        D1 d{};
        d.N = N; d.H = H; d.B = B; d.T = T; d.HT = HT; d.NB = NB; d.NW = BP_NW; d.TPW = 1; d.G = G; d.TG = TG;
        d.nblk = nblk; d.ntg = ntg; d.Bt = 16 * ntg; d.nvec = NVEC_BP; d.BN = (long long)B * N; d.HC = 1; d.Hc = H;
        *out = d;
        return true;
    }
    return false;
}

bool plan_bp(int N, int H, int B, int T, int /* control: a fixed grid has no controller */, int method, D1 *out)
{
    if (method == PHX_DOPRI5) return false;
    return plan_bp_cus(num_cus(), N, H, B, T, out);
}

Regions make_layout_bp(const D1 &d, bool grads)
{
    Regions L{};
    Take take;
    const size_t R = (size_t)d.ntg * 4 * d.HT * 4;
    L.cnt = take(4096);
    L.part = take((size_t)d.TG * d.G * R * 64 * 8);
    L.zbuf = take((size_t)d.TG * R * 64 * 8);
    L.xbytes = take.off - L.part;                           // granule buffers are zeroed before every launch
    L.scratch = take((size_t)d.TG * d.G * NVEC_BP * d.ntg * d.NB * 512 * 4);
    L.pp = (long long)align_up((size_t)4 * d.H * d.N + d.N + 2 * d.H, 4);
    L.nparts = d.TG * BP_NW;
    L.dtheta = take(grads ? (size_t)L.pp * 4 * L.nparts : 0);   // zeroed before every launch: the kernel only adds
    L.prof = take(0);
    L.wimg = take((size_t)d.nblk * blk_floats_ch(d.HT, d.H) * 4);
    L.hq = take(grads ? (size_t)d.TG * d.G * BP_NW * 4 * 4 * d.HT * 256 * 4 : 0);
    L.total = take.off;
    return L;
}

const void *prepare_bp(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    if (p->wimg) a.w.wimg = (const float *)p->wimg;   // packed once by the caller for these parameter values
    else
        hipLaunchKernelGGL(k1_pack_images, dim3(d.nblk), dim3(256), 0, st, to_net(p), (float *)a.w.wimg, d.HT, 1, p->H,
                           blk_floats_ch(d.HT, p->H));
    a.lds = (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + BP_LDS_TAIL;
    return d.HT == 3 ? reinterpret_cast<const void *>(k1_solve_bp<3>) : reinterpret_cast<const void *>(k1_solve_bp<8>);
}

hipError_t launch_bp(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_plain(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.t, a.y_saved, a.grad_y,
                        a.adj_y0, a.status, a.nfe, a.nsteps, a.grads, a.PP, a.ckpt);
}

bool reduce_bp(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st)
{
    return launch_reduce_grads(a.w.dtheta, npart, a.PP, a.d.N, a.d.H, g, overwrite, st);
}

}  // namespace

namespace phxh {
const Backend &bp_backend()
{
    static const Backend b = {5, false, true, false, plan_bp, make_layout_bp, plan6_ht, prepare_bp, launch_bp, reduce_bp, true};
    return b;
}

// rows per launch of a batch of B (0: no plan); cus <= 0: sized for the 256 CUs of an MI355X (no device in sight)
int bp_chunk(int cus, int N, int H, int B, int T)
{
    if (cus <= 0) cus = 256;
    D1 d;
    if (plan_bp_cus(cus, N, H, B, T, &d)) return B;
    for (int bc = 4096; bc >= 16; bc >>= 1)
        if (bc < B && plan_bp_cus(cus, N, H, bc, T, &d)) return bc;
    return 0;
}

// the plan of ONE launch of B rows on `cus` CUs (diagnostic: phx_debug_backprop_plan)
bool bp_plan(int cus, int N, int H, int B, int T, D1 *out)
{
    return plan_bp_cus(cus, N, H, B, T, out);
}

// workspace bytes in front of the checkpoint region: the largest layout among the launches of the batch
size_t bp_base_bytes(int cus, int N, int H, int B, int T)
{
    if (cus <= 0) cus = 256;
    const int chunk = bp_chunk(cus, N, H, B, T);
    if (chunk <= 0) return 0;
    size_t need = 0;
    for (const int bc : {chunk, B % chunk}) {
        D1 d;
        if (bc > 0 && plan_bp_cus(cus, N, H, bc, T, &d)) need = std::max(need, make_layout_bp(d, true).total);
    }
    return need;
}
}  // namespace phxh
