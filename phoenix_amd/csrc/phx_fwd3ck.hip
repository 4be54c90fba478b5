// phx_fwd3ck.hip -- the CALLS + CLAMP forms of k1_solve_fwd3c (phx_mfma_fwd3c.inc): several shared-control calls per
// launch, each with a set of up to PHX_CLAMP_MAX genes held at their initial values (phx_odeint_clamped_sets).  A
// translation unit of its own: the six forms are compiled beside those of phx_fwd3c.hip instead of after them.
// phx_fwd3c.hip plans, lays out and launches them.
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

namespace phxh {
// nbt: (tile, block) slots per wave the form is built for (1 or 8), as prepare_fwd3c picks it
const void *fwd3c_clamp_kernel(int nbt, bool half, bool hb)
{
    switch (nbt * 2 + (half ? 1 : 0) + (hb ? 32 : 0)) {
    case 35: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, true, true, true>);
    case 34: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, true, true, true>);
    case 3: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, true, false, true, true>);
    case 2: return reinterpret_cast<const void *>(k1_solve_fwd3c<1, false, false, true, true>);
    case 17: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, true, false, true, true>);
    default: return reinterpret_cast<const void *>(k1_solve_fwd3c<8, false, false, true, true>);
    }
}
}  // namespace phxh
