"""CPU-only checks of the per-row clamp's boundaries (phx_odeint_clamped_rows,
phx_odeint_adjoint_backward_clamped_rows and their size query, include/phoenix_hip.h; the `clamp=` keyword of `odeint`,
`odeint_adjoint` and `odeint_per_sample`): the symbols exist and agree with the header, every argument check answers
before a device call, the size query is 0 exactly where the launch is not served, and the list is checked on the host."""
import ctypes as C
import os
import re

import pytest
import torch

from test_abi_cpu import _declared_symbols

BAD_ARG = 4
NEW = ("phx_odeint_clamped_rows_workspace_bytes", "phx_odeint_clamped_rows", "phx_odeint_adjoint_backward_clamped_rows",
       "phx_debug_clamped_rows_plan")


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phoenix_hip.h")).read()


def test_new_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in NEW:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change
    assert set(mod.EXPORTS) == set(_declared_symbols())


def test_prototypes_agree_with_the_header():
    """the number of parameters the header declares is the number of ctypes argtypes, and the list comes with its width"""
    mod, lib = _lib()
    src = _header()
    for name in NEW:
        m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(getattr(lib, name).argtypes), (name, args)
    for name in NEW[1:3]:
        m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S).group(1)
        assert re.search(r"const int \*clamp_genes,\s*int width", m), name
    assert lib.phx_odeint_clamped_rows_workspace_bytes.restype is C.c_size_t


def test_size_query_is_zero_exactly_where_the_launch_is_not_served(monkeypatch):
    mod, lib = _lib()
    from phoenix_amd import engine
    f = lib.phx_odeint_clamped_rows_workspace_bytes
    for op in (mod.OP_ODEINT, mod.OP_ADJOINT):
        assert f(op, 96, 8, 5, 3) > 0 and f(op, 350, 40, 150, 3) > 0
        assert f(op, 96, 48, 5, 3) > 0
        assert f(op, 96, 56, 5, 3) == 0 and f(op, 96, 49, 5, 3) == 0          # H > 48
        for shape in ((0, 8, 5, 3), (96, 0, 5, 3), (96, 8, 0, 3), (96, 8, 5, -1)):
            assert f(op, *shape) == 0, shape
        # a fixed-grid method has no per-row kernel: the engine's query, which knows the method, says so
        for m in ("euler", "midpoint", "rk4"):
            assert engine.clamped_rows_plan_exists(op, 96, 8, 5, 3, m) == 0
        assert engine.clamped_rows_plan_exists(op, 96, 8, 5, 3, "dopri5") == f(op, 96, 8, 5, 3)
    assert f(mod.OP_RHS_FORWARD, 96, 8, 5, 3) == 0 and f(mod.OP_RHS_VJP, 96, 8, 5, 3) == 0
    # the backward launch is k1_solve_adj3's at every group size, also where an unclamped solve takes k1_solve_adj2
    plan = (C.c_int * 8)()
    assert lib.phx_debug_clamped_rows_plan(mod.OP_ADJOINT, 96, 8, 5, 3, plan) == 1 and plan[0] == 3
    assert lib.phx_debug_clamped_rows_plan(mod.OP_ADJOINT, 96, 56, 5, 3, plan) == 0 and list(plan) == [0] * 8
    monkeypatch.setenv("PHX_ENGINE", "v0")
    for op in (mod.OP_ODEINT, mod.OP_ADJOINT):
        assert f(op, 96, 8, 5, 3) == 0
        assert engine.clamped_rows_plan_exists(op, 96, 8, 5, 3) == 0           # (the plan switches are part of its key)


def _call(lib, mod, backward, N=96, H=8, B=5, T=3, method="dopri5", control=None, clamp=0x5000, width=2, a=0x1000, t=0x2000,
          b=0x3000, ws=0x4000, opts=True, calls=1):
    """either entry point with made-up device addresses: only calls that must return before touching the device"""
    x = C.cast((C.c_float * 4)(), C.c_void_p)
    prm = mod.PhxParams(x, x, x, x, x, x, N, H, None)
    o = mod.PhxSolveOpts(mod.METHODS[method], mod.CTRL_PER_TRAJECTORY if control is None else control, 1e-7, 1e-9, 1, 0, 0,
                         calls, 0)
    op = C.byref(o) if opts else None
    if backward:
        return lib.phx_odeint_adjoint_backward_clamped_rows(C.byref(prm), t, B, T, op, clamp, width, a, b, 0x3800, None, 0x6000,
                                                            0x6100, 0x6200, ws, 1 << 30, None)
    return lib.phx_odeint_clamped_rows(C.byref(prm), a, t, B, T, op, clamp, width, b, 0x6000, 0x6100, 0x6200, ws, 1 << 30, None)


@pytest.mark.parametrize("backward", [False, True])
def test_entry_points_reject_bad_arguments_before_any_device_call(monkeypatch, backward):
    mod, lib = _lib()
    for width in (0, -1, 5, 1 << 20):
        assert _call(lib, mod, backward, width=width) == BAD_ARG, width
    for width in (1, 2, 3, 4):
        assert _call(lib, mod, backward, width=width, clamp=None) == BAD_ARG, width
    for m in ("euler", "midpoint", "rk4"):
        assert _call(lib, mod, backward, method=m) == BAD_ARG, m
    assert _call(lib, mod, backward, control=mod.CTRL_SHARED) == BAD_ARG
    assert _call(lib, mod, backward, H=56) == BAD_ARG                      # a shape whose size query is 0
    assert _call(lib, mod, backward, B=0) == BAD_ARG and _call(lib, mod, backward, T=0) == BAD_ARG
    assert _call(lib, mod, backward, a=None) == BAD_ARG and _call(lib, mod, backward, t=None) == BAD_ARG
    assert _call(lib, mod, backward, b=None) == BAD_ARG and _call(lib, mod, backward, ws=None) == BAD_ARG
    assert _call(lib, mod, backward, opts=False) == BAD_ARG
    monkeypatch.setenv("PHX_ENGINE", "v0")
    assert _call(lib, mod, backward) == BAD_ARG


# --------------------------------------------------------------------------- the list, checked on the host
def _net(N=16, H=4):
    import phoenix_amd
    return phoenix_amd.ODENet("cpu", N, neurons=H)


def _fns():
    import phoenix_amd
    return (("odeint", phoenix_amd.odeint), ("odeint_adjoint", phoenix_amd.odeint_adjoint),
            ("odeint_per_sample", phoenix_amd.odeint_per_sample))


BAD_LISTS = [([0, 1], ValueError, "rows"),                       # two entries for three rows
             ([0, [1, 2, 3, 4, 5], 2], ValueError, "at most 4"),  # a set of five
             ([0, 1, 16], ValueError, "not a gene"),              # N = 16: the last gene is 15
             ([0, -2, 1], ValueError, "not a gene"),              # -1 alone means none
             ([0, 1.5, 2], TypeError, "integers"), (torch.tensor([0.0, 1.0, 2.0]), TypeError, "integer tensor"),
             ([0, True, 2], TypeError, "integers"), (7, TypeError, "sequence"),
             (torch.zeros(3, 5, dtype=torch.int64), ValueError, "at most 4")]


@pytest.mark.parametrize("clamp,exc,what", BAD_LISTS)
def test_the_list_is_checked_on_the_host_with_messages_that_name_the_function(clamp, exc, what):
    y0, t = torch.zeros(3, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64).repeat(3, 1)
    for name, fn in _fns():
        with pytest.raises(exc, match=r"%s: .*%s" % (name, what)):
            fn(_net(), y0, t, clamp=clamp)


def test_shared_control_with_a_held_gene_points_at_odeint_calls():
    import phoenix_amd
    y0, t = torch.zeros(3, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64)
    for fn in (phoenix_amd.odeint, phoenix_amd.odeint_adjoint):
        with pytest.raises(ValueError, match="odeint_calls"):
            fn(_net(), y0, t, clamp=[0, -1, 3])                                           # t [T]: one shared controller
        with pytest.raises(ValueError, match="odeint_calls"):
            fn(_net(), y0, t, clamp=[0, -1, 3], options={"batch_control": "shared"})
    # an all-empty list holds nothing: it is the unclamped call, whose next requirement is the GPU
    for clamp in ([-1, -1, -1], [(), [], -1], torch.full((3, 2), -1)):
        with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
            phoenix_amd.odeint(_net(), y0, t, clamp=clamp)


def test_good_lists_reach_the_device_requirement():
    """duplicates count once, a tensor padded with -1, numpy-free nested forms: the next thing asked for is the GPU"""
    import phoenix_amd
    from phoenix_amd.odeint import _clamp_list, _row_clamp
    y0, t = torch.zeros(3, 1, 16), torch.linspace(0, 1, 4, dtype=torch.float64).repeat(3, 1)
    pad = torch.tensor([[0, 15, -1, -1], [-1, -1, -1, -1], [3, 2, 1, 0]], dtype=torch.int32)
    assert _clamp_list(pad, 3, 16, who="odeint", unit="row") == [(0, 15), (), (0, 1, 2, 3)]
    assert _clamp_list([[5, 5, 4, 5], -1, (7, -1)], 3, 16, who="odeint", unit="row") == [(4, 5), (), (7,)]
    held = _row_clamp("odeint", _net(), y0, t, {}, [[5, 5, 4], 2, [5, 4]])
    assert held.sets == [(4, 5), (2,), (4, 5)]
    assert held.groups == [((2,), [1]), ((4, 5), [0, 2])]               # rows grouped by set, in sorted order of the sets
    assert held.device_list(torch.device("cpu")).tolist() == [[4, 5], [2, -1], [4, 5]]
    assert _row_clamp("odeint", _net(), y0, t, {}, [-1, (), []]) is None and _row_clamp("odeint", _net(), y0, t, {}, None) is None
    for name, fn in _fns():
        for clamp in (pad, [[5, 5, 4, 5], -1, (7, -1)], [0, -1, 15], torch.tensor([0, -1, 15])):
            with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
                fn(_net(), y0, t, clamp=clamp)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.odeint(_net(), y0, t[0], clamp=[0, -1, 15], options={"batch_control": "per_trajectory"})


def test_the_new_units_are_built_and_listed():
    from phoenix_amd import build
    names = [os.path.basename(s) for s in build.sources()]
    for unit in ("phx_fwd3r.hip", "phx_adj3r.hip"):
        assert unit in names and unit in build.LISTINGS
    # the forward forms are k1_solve_fwd3's: the unit is compiled with phx_fwd3.hip's flags
    assert build.UNIT_FLAGS["phx_fwd3r.hip"] == build.UNIT_FLAGS["phx_fwd3.hip"]
    assert "phx_adj3r.hip" not in build.UNIT_FLAGS and "phx_adj3.hip" not in build.UNIT_FLAGS
