"""The planner on the device: no launches, only queries."""
import ctypes as C

import pytest

from test_plans_cpu import T, lib, pt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", (2, 3))
@pytest.mark.parametrize("shape", ((350, 40, 17), (2000, 120, 23), (700, 200, 33)))
def test_debug_plan_at_the_devices_cu_count_is_the_plan_the_solves_run(pt, lib, op, shape):
    """phx_debug_plan for the first kernel of the direction = what phx_debug_profile_region reports for the device"""
    N, H, B = shape
    cus = lib.phx_device_cus()
    assert cus > 0
    lib.phx_debug_profile_region.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for ctl in (0, 1):
        off, nwg, plan6 = C.c_size_t(0), C.c_int(0), (C.c_int * 6)()
        assert lib.phx_debug_profile_region(op, N, H, B, T, ctl, C.byref(off), C.byref(nwg), plan6) == 0
        kernel = (lib.phx_debug_forward_kernel_m if op == pt.ODEINT else lib.phx_debug_adjoint_kernel_m)(N, H, B, T, ctl, 3)
        first = [k for o, k in pt.KERNELS if o == op and k != 5 and pt.plan(lib, o, k, cus, N, H, B, ctl, 3)][0]
        assert first == kernel
        p = dict(zip(pt.FIELDS, pt.plan(lib, op, first, cus, N, H, B, ctl, 3)))
        assert (p["NW"], p["TPW"], p["NB"], p["G"], p["TG"]) == tuple(plan6[:5])
        assert plan6[5] == (p["HC"] * 10 + p["res"] + 2 * p["hb"] + (4 if p["split"] > 1 else 0) if first == 4 else p["HT"])
        assert (off.value, nwg.value) == (p["prof"], p["TG"] * p["G"])
    # ... and the workspace query covers the remainder launch of a batch that runs in chunks (6000 genes, 200 hidden rows,
    # 673 .. 686 trajectories: the remainder's layout was once larger than the query's answer)
    for B in range(673, 687) if shape[1] == 200 else ():
        k = (lib.phx_debug_forward_kernel_m if op == pt.ODEINT else lib.phx_debug_adjoint_kernel_m)(6000, 200, B, T, 1, 3)
        launches = lib.phx_debug_solve_launches(op, 6000, 200, B, T, 1, 3)
        chunk = next(c for c in [B] + [1 << i for i in range(12, 3, -1)] if (B + c - 1) // c == launches)
        for rows in (chunk, B % chunk):
            if rows:
                v = pt.plan(lib, op, k, cus, 6000, 200, rows, 1, 3)
                assert v and v[pt.FIELDS.index("total")] <= lib.phx_workspace_bytes(op, 6000, 200, B, T), (B, rows)
