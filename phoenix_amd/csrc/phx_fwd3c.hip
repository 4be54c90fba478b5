// phx_fwd3c.hip -- translation unit of the third-generation forward solve for wide hidden layers (k1_solve_fwd3c,
// phx_mfma_fwd3c.inc: hidden chunks of <= 48 rows): launch planning, workspace layout and the host entry points the C ABI
// (phx_engine.hip) calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "phx_solver.hpp"
#include "phx_host.hpp"

using namespace phxh;

#include "phx_mfma_common.inc"
#include "phx_mfma_v3common.inc"
#include "phx_mfma_fwd3c.inc"
#include "phx_plan.hpp"

namespace {

// plan_chunked with the forward kernel's rules: up to eight slots per wave, groups of several tiles on half the chip
bool plan_fwd3c(const Shape &s, D1 *out)
{
    if (!chunked_shape(s)) return false;
    const Switches sw = read_switches(SW_FWD | SW_CHUNKED);
    if (sw.v0 || sw.fwd_v1 || sw.v3c_off) return false;
    return plan_chunked(s, sw, ChunkedRules{NVEC_FWD3C, 8, 2, true, HSF_BYTES}, ctlf3c_bytes,
                        [](int Bt, int ntg, int parts) { return hsf_offset(Bt, ntg) + spf_bytes(ntg, parts); }, out);
}

Regions make_layout_f3c(const D1 &d, bool)
{
    LayoutSpec s;
    s.part_rows = s.zbuf_rows = (size_t)d.ntg * d.HC * 2 * d.HT * 4 + d.ntg;   // hidden rows of every chunk + norm rows per group
    s.two_sets = true;
    return make_regions(d, s);
}

size_t lds_bytes_fwd3c(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.Hc) * 4 * d.NB * (d.res ? d.HC : 1) +
           (d.hb ? hsf_offset(d.Bt, d.ntg) + HSF_BYTES
                 : (d.split > 1 ? hsf_offset(d.Bt, d.ntg) + spf_bytes(d.ntg, d.split) : ctlf3c_bytes(d.Bt, d.ntg)));
}

const void *prepare_fwd3c(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    // the chunk images of this kernel family (three-tile chunks) are not the caller's phx_params.wimg format for H > 48
    // (one eight-tile chunk / seven-tile 100-row chunks): packed per launch from the parameter tensors
    pack_images(a, p, st, false);
    // (tile, block) slots per wave the kernel is built for (unused slots of the eight-slot form cost a scalar branch each)
    const int nbt = d.TPW * d.NB <= 1 || d.split > 1 ? 1 : 8;
    const bool half = d.Hc <= 40;   // every chunk's last tile has at most 8 live rows (rho16, phx_mfma_v3common.inc)
    if (a.clamp) return d.Bcall > 0 ? fwd3c_clamp_kernel(nbt, half, d.hb != 0) : nullptr;   // held genes per call (phx_fwd3ck.hip)
    if (d.Bcall > 0)   // several calls, a time row each (one call alone is an ordinary shared-control launch)
        switch (nbt * 2 + (half ? 1 : 0) + (d.hb ? 32 : 0)) {
        case 35: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, true, true>);
        case 34: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, true, true>);
        case 3: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, false, true>);
        case 2: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, false, true>);
        case 17: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, true, false, true>);
        default: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, false, false, true>);
        }
    switch (nbt * 2 + (half ? 1 : 0) + (d.hb ? 32 : 0)) {
    case 35: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, true>);
    case 34: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, true>);
    case 3: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, false>);
    case 2: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, false>);
    case 17: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, true, false>);
    default: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, false, false>);
    }
}

hipError_t launch_fwd3c(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.y0, a.t, a.sol,
                             a.status, a.nfe, a.nsteps, a.clamp, a.clamp_width);
}

}  // namespace

namespace phxh {
const Backend &fwd3c_backend()
{
    static const Backend b = {4, true, false, true,
                                    plan_fwd3c, make_layout_f3c, lds_bytes_fwd3c, plan6_chunked, prepare_fwd3c, launch_fwd3c, nullptr};
    return b;
}
}  // namespace phxh
