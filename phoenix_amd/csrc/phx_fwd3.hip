// phx_fwd3.hip -- translation unit of the third-generation forward solve (k1_solve_fwd3, phx_mfma_fwd3.inc): launch
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
#include "phx_mfma_v3common.inc"
#include "phx_mfma_fwd3.inc"
#include "phx_plan.hpp"

namespace {

size_t lds_bytes_fwd3(const D1 &d)
{
    return (size_t)blk_floats_ch(d.HT, d.H) * 4 * d.NB + ((ctlf3_bytes(d.Bt, d.ntg) + 15) & ~(size_t)15) +
           (v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1 ? v3_comb_bytes(d.NW, 2 * d.HT) : 0);
}

// plan_resident for dopri5 with H <= 48.  One wave per SIMD (NW <= 4).  The eight-wave form (two waves per SIMD under a
// 256-register cap) computed wrong step sizes in round 3 -- the store-data hazard of phx_mfma_v3common.inc, not the form
// itself: rebuilt in round 4 with the guarded stores it passes the parity suite, and it is no faster at C4 (0.266-0.268 ms
// against 0.268-0.270: 38-148 spilled registers, twice the exchange members per group), so it is not built.
bool plan_fwd3(const Shape &s, D1 *out)
{
    if (s.cus <= 0 || s.method != PHX_DOPRI5 || s.H > 48) return false;
    const Switches sw = read_switches(SW_FWD | SW_MAXNW | SW_V3_NB);
    if (sw.v0 || sw.fwd_v1) return false;
    const int HT = 3;
    // (control LDS + that of the block-split combine where the batch is that small: v3_split_parts)
    return plan_resident(s, make_tiles(HT, 1, s.H, NVEC_FWD3), std::min(4, sw.v1_maxnw), 4, sw.v3_nb,
                         [&](int NW, int TPW, int TG, int ntg, int Bt) {
                             return ((ctlf3_bytes(Bt, ntg) + 15) & ~(size_t)15) +
                                    (v3_split_parts(TG, NW, TPW, ntg) > 1 ? v3_comb_bytes(NW, 2 * HT) : 0);
                         }, out);
}

Regions make_layout_f3(const D1 &d, bool)
{
    LayoutSpec s;
    s.part_rows = s.zbuf_rows = (size_t)d.ntg * 2 * d.HT * 4 + d.ntg;   // hidden rows + norm rows per group
    s.two_sets = true;
    return make_regions(d, s);
}

const void *prepare_fwd3(SolveArgs &a, const phx_params *p, hipStream_t st)
{
    const D1 &d = a.d;
    pack_images(a, p, st);
    // HALF: the last hidden tile has at most 8 live rows (H <= 40 with three tiles; rho16 in phx_mfma_v3common.inc)
    const char *eh = getenv("PHX_V3_HALF");   // diagnostic: 0 = full last tile also where half of it is padding
    const bool half = p->H <= 16 * (d.HT - 1) + 8 && !(eh && eh[0] == '0');
    const char *et = getenv("PHX_V3_TERM");   // diagnostic: 0 = no terminal tiles, every step ends with the accept pass
    a.w.prof_level = (a.w.prof_level & 0xff) | ((et && et[0] == '0') ? FWD3_NO_TERM : 0);
    const bool split = v3_split_parts(d.TG, d.NW, d.TPW, d.ntg) > 1;   // small batch: the waves of a tile split its blocks
    // held genes per call (phx_fwd3k.hip), or per trajectory row under per-trajectory control (phx_fwd3r.hip)
    if (a.clamp) return d.Bcall > 0 ? fwd3_clamp_kernel(half) : fwd3_rows_kernel(half, split);
    if (d.Bcall > 0)   // several calls, a time row each (one call alone is an ordinary shared-control launch)
        return half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false, true>)
                    : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false, true>);
    return split ? (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, true>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, true>))
                 : (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false>));
}

hipError_t launch_fwd3(const void *fn, const SolveArgs &a, hipStream_t st)
{
    return launch_persistent(fn, dim3(a.d.TG * a.d.G), dim3(64 * a.d.NW), a.lds, st, a.net, a.d, a.w, a.cfg, a.y0, a.t, a.sol,
                             a.status, a.nfe, a.nsteps, a.clamp, a.clamp_width);
}

}  // namespace

namespace phxh {
const Backend &fwd3_backend()
{
    static const Backend b = {3, true, false, true, plan_fwd3, make_layout_f3, lds_bytes_fwd3, plan6_ht, prepare_fwd3,
                              launch_fwd3, nullptr};
    return b;
}
}  // namespace phxh
