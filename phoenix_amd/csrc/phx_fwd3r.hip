// phx_fwd3r.hip -- the CLAMP forms of k1_solve_fwd3 (phx_mfma_fwd3.inc) without CALLS: per-trajectory step control, every
// trajectory row with a set of up to PHX_CLAMP_MAX genes of its own held at their initial values
// (phx_odeint_clamped_rows).  A translation unit of its own, beside phx_fwd3k.hip and with phx_fwd3.hip's flags
// (phoenix_amd/build.py): the forms of the other units compile as before.  phx_fwd3.hip plans, lays out and launches them.
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

namespace phxh {
const void *fwd3_rows_kernel(bool half, bool split)
{
    return split ? (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, true, false, true>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, true, false, true>))
                 : (half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false, false, true>)
                         : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false, false, true>));
}
}  // namespace phxh
