"""CPU checks of the calls-with-their-own-grids form of phx_odeint: the new exports plan without a device (sized for 256
CUs), the older query is unchanged, the combination is refused where it always was."""
import ctypes as C

from phoenix_amd import _lib

DOPRI5, RK4 = _lib.METHODS["dopri5"], _lib.METHODS["rk4"]


def test_new_exports_plan_the_dopri5_kernels_without_a_device():
    lib = _lib.load()
    assert lib.phx_abi_version() == 7
    for (N, H, Bc, T, m, kern) in [(11165, 40, 60, 10, DOPRI5, 3), (14691, 200, 24, 10, DOPRI5, 4), (700, 20, 20, 10, RK4, 1)]:
        for K in (2, 7, 300):
            B = Bc * K
            assert lib.phx_odeint_calls_grids_workspace_bytes(N, H, B, T, K, m) > 0
            assert lib.phx_debug_calls_grids_kernel_m(N, H, B, T, K, m) == kern
            plan = (C.c_int * 6)()
            n = lib.phx_debug_calls_grids_plan(N, H, B, T, K, m, plan)
            assert 1 <= n <= K
            kernel, TG, G, NW, ntg, cus = list(plan)
            assert kernel == kern and TG == n and cus == 256 and TG * G <= 256      # every workgroup resident
            assert 16 * ntg >= Bc and 1 <= NW <= 8                                    # a call is one group
            assert lib.phx_debug_calls_grids_launches(N, H, B, T, K, m) == -(-K // n)
    assert lib.phx_odeint_calls_grids_workspace_bytes(350, 40, 60, 10, 7, DOPRI5) == 0     # 60 rows are not 7 equal calls
    assert lib.phx_debug_calls_grids_kernel_m(350, 40, 60, 10, 7, DOPRI5) == 0


def test_shared_grid_query_is_unchanged():
    lib = _lib.load()
    assert lib.phx_odeint_calls_workspace_bytes(350, 40, 60, 10, 7) == 0
    assert lib.phx_odeint_calls_workspace_bytes(350, 40, 60, 10, 6) == lib.phx_odeint_calls_workspace_bytes(350, 40, 60, 10, 6)


def test_one_call_with_a_grid_per_sample_is_still_refused():
    """phx_odeint: shared control + t_per_sample is PHX_ERR_BAD_ARG unless calls > 1 (checked before any device call)"""
    lib = _lib.load()
    x = (C.c_float * 64)()
    prm = _lib.PhxParams(*([C.cast(x, C.c_void_p)] * 6), 4, 2, None)
    for calls, step, want_bad in ((0, 0.0, True), (1, 0.0, True), (2, 0.5, True)):
        o = _lib.PhxSolveOpts(RK4, _lib.CTRL_SHARED, 1e-7, 1e-9, 1, 0, 0, calls, 0)
        rc = lib.phx_odeint_stepped(C.byref(prm), x, x, 4, 2, C.byref(o), x, x, x, x, x, 64, None, step)
        assert (rc == 4) == want_bad, (calls, step, rc)
