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
#include "phx_plan.hpp"

namespace {

constexpr size_t BP_LDS_TAIL = 256;

size_t lds_bytes_bp(const D1 &d) { return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + BP_LDS_TAIL; }

// Four waves per workgroup, one trajectory tile each; the smallest NB (gene blocks per workgroup) whose grid the device
// holds at once: no search over waves and no cost, so not a case of plan_resident.  H <= 128: the weight images of a
// gene block stay LDS resident, like k1_solve_adj2.  A fixed grid has no controller: `control` is not looked at.
bool plan_bp(const Shape &s, D1 *out)
{
    if (s.method == PHX_DOPRI5 || s.calls > 1) return false;
    if (s.cus <= 0 || s.N <= 0 || s.H <= 0 || s.H > 128 || s.B <= 0 || read_switches(0).v0) return false;
    const Tiles t = make_tiles(s.H <= 48 ? 3 : 8, 1, s.H, NVEC_BP);
    if (t.blkbytes + BP_LDS_TAIL > LDS_BUDGET) return false;
    const int nblk = (s.N + 31) / 32, ntt = (s.B + 15) / 16;
    const int TG = (ntt + BP_NW - 1) / BP_NW;
    const int NBmax = (int)std::min<size_t>((LDS_BUDGET - BP_LDS_TAIL) / t.blkbytes, 8);
    for (int NB = 1; NB <= NBmax; ++NB) {
        if ((long long)TG * ((nblk + NB - 1) / NB) > s.cus) continue;
        *out = make_d1(s, t, BP_NW, 1, NB, TG, TG == 1 ? ntt : BP_NW, false);
        return true;
    }
    return false;
}

Regions make_layout_bp(const D1 &d, bool grads)
{
    LayoutSpec s;
    s.part_rows = s.zbuf_rows = (size_t)d.ntg * 4 * d.HT * 4;
    s.prof = false;
    s.tail = true;
    s.pp = (long long)align_up((size_t)4 * d.H * d.N + d.N + 2 * d.H, 4);
    s.nparts = d.TG * BP_NW;
    s.dtheta = grads ? (size_t)s.pp * 4 * s.nparts : 0;   // zeroed before every launch: the kernel only adds
    s.has_hq = true;
    s.hq = grads ? (size_t)d.TG * d.G * BP_NW * 4 * 4 * d.HT * 256 * 4 : 0;
    return make_regions(d, s);
}

const void *prepare_bp(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    pack_images(a, p, st);
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
    static const Backend b = {5, false, true, false, plan_bp, make_layout_bp, lds_bytes_bp, plan6_ht, prepare_bp, launch_bp,
                              reduce_bp, true};
    return b;
}
}  // namespace phxh
