// phx_fwd3k.hip -- the CALLS + CLAMP forms of k1_solve_fwd3 (phx_mfma_fwd3.inc): several shared-control calls per launch,
// each with a set of up to PHX_CLAMP_MAX genes held at their initial values (phx_odeint_clamped_sets).  A translation
// unit of its own: the forms are compiled beside those of phx_fwd3.hip, with that unit's flags (phoenix_amd/build.py),
// instead of after them.  phx_fwd3.hip plans, lays out and launches them.
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
const void *fwd3_clamp_kernel(bool half)
{
    return half ? reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, true, false, true, true>)
                : reinterpret_cast<const void *>(k1_solve_fwd3<3, 256, false, false, true, true>);
}
}  // namespace phxh
