"""CPU-only checks of the total-effects network at a fixed point (phoenix_amd.steady_state_response):
`steady_state_response_reference`, the numpy restatement that tests/test_steady_response_gpu.py holds the device to, is
pinned here to the dense N x N formulas and to central differences of `steady_states_reference`; the symbols exist and the
argument checks answer before any device call.  Models and float64 helpers: tests/test_steady_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols
from test_steady_cpu import C64, SHAPES, moving, reference

BAD_ARG, WORKSPACE = 4, 5
NAMES = ("phx_steady_inverse_workspace_bytes", "phx_steady_inverse", "phx_steady_response_factors", "phx_steady_response")


def singular_model():
    """(params, y [3, 6]) with H = 1 whose middle row has S[0, 0] = 1 and S[1, 0] = 0 exactly, in float32 as in float64: only
    gene 0 feeds hidden unit 0 back (Wa[n, 0] = 0 for n > 0, Wa[0, 0] = Ws[0, 0] = 1, Wp[0, 0] = 0) and a'(0.5) = 1, so the
    first column of I - S is zero there; the other rows have y[b, 0] != 0.5"""
    r = np.random.default_rng(5)
    N = 6
    p = {"Ws": r.normal(0, 0.5, (1, N)), "Wp": r.normal(0, 0.5, (1, N)), "Wa": r.normal(0, 0.4, (N, 2)),
         "bs": r.uniform(-.1, .1, 1), "bp": r.uniform(-.1, .1, 1), "g": r.uniform(0.2, 1.2, N)}
    p["Ws"][0, 0], p["Wp"][0, 0], p["Wa"][0, 0], p["Wa"][1:, 0] = 1.0, 0.0, 1.0, 0.0
    y = r.random((3, N))
    y[:, 0] = (0.25, 0.5, 0.875)
    return {k: v.astype(np.float32) for k, v in p.items()}, y.astype(np.float32)


def some_regulators(p, held, free, b, n=3):
    """for row b: n moving genes, then the row's held genes and one gene that never moves"""
    N = free.shape[1]
    rng = np.random.default_rng(100 + b + N)
    mov = [int(k) for k in rng.choice(np.nonzero(free[b])[0], n, replace=False)]
    dead = int(np.nonzero(p["g"] <= 0)[0][0])
    return mov, mov + [int(k) for k in held[b]] + [dead]


def row_response(pa, p, y, held, b, regs, input):
    """the reference on row b alone with reduce="mean": response[i, j] is the row's own entry"""
    out = pa.steady_state_response_reference(p, y[b:b + 1], clamp=[held[b]], regulators=regs, input=input, reduce="mean")
    assert np.all(out.info == 0), out.info                     # the row is used: the comparison is not vacuous
    assert out.response.dtype == np.float64 and out.response.shape == (len(out.regulators), y.shape[1])
    return out.response


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_production_form_equals_the_dense_inverse(N, H, B):
    import phoenix_amd as pa
    p, y0, held, ref = reference(N, H, B)
    free = moving(p, held, B)
    wa = p["Wa"].astype(np.float64)
    worst = 0.0
    for b in range(B):
        m = free[b].astype(np.float64)
        dense = np.linalg.inv(np.eye(N) - m[:, None] * (wa @ C64(p, ref.y, b))) * m[None, :]      # R[j, i]
        got = row_response(pa, p, ref.y, held, b, None, "production")
        worst = max(worst, float(np.abs(got - dense.T).max()))
        assert not got[~free[b]].any()                          # a regulator that does not move: an exact zero row
        assert not got[:, ~free[b]].any()                       # ... and a target that does not move: an exact zero column
    print("(%d, %d, %d): |Woodbury - dense (I - M Wa C)^-1 M| %.1e" % (N, H, B, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_level_form_equals_the_dense_solve_with_the_gene_held(N, H, B):
    import phoenix_amd as pa
    p, y0, held, ref = reference(N, H, B)
    free = moving(p, held, B)
    wa = p["Wa"].astype(np.float64)
    worst, low = 0.0, np.inf
    for b in range(B):
        _, regs = some_regulators(p, held, free, b)
        got = row_response(pa, p, ref.y, held, b, regs, "level")
        J = wa @ C64(p, ref.y, b)
        prod = row_response(pa, p, ref.y, held, b, regs, "production")
        for i, k in enumerate(regs):
            m = free[b].astype(np.float64)
            m[k] = 0.0
            want = np.linalg.solve(np.eye(N) - m[:, None] * J, m * J[:, k])
            want[k] = 1.0
            worst = max(worst, float(np.abs(got[i] - want).max()))
            assert got[i, k] == 1.0
            if free[b, k]:
                low = min(low, abs(prod[i, k]))                 # |R[k, k]|
    print("(%d, %d, %d): |R[:, k] / R[k, k] - dense solve with k held| %.1e, |R[k, k]| >= %.2f" % (N, H, B, worst, low))
    assert worst <= 1e-12


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_level_form_equals_a_central_difference_of_the_steady_states(N, H, B):
    """y*(level of k = y*_k +- eps) by `steady_states_reference` with k held, eps = 1e-4, three moving genes per row; only rows
    whose held set then has at most four genes"""
    import phoenix_amd as pa
    p, y0, held, ref = reference(N, H, B)
    free = moving(p, held, B)
    eps, worst, rows = 1e-4, 0.0, [b for b in range(B) if len(held[b]) <= 3]
    assert rows
    picks = {b: some_regulators(p, held, free, b)[0] for b in rows}
    for pick in range(3):
        ends = []
        for sign in (1.0, -1.0):
            start = ref.y[rows].copy()
            for at, b in enumerate(rows):
                start[at, picks[b][pick]] += sign * eps
            clamp = [tuple(held[b]) + (picks[b][pick],) for b in rows]
            out = pa.steady_states_reference(p, start, clamp=clamp, tol=1e-13, max_iter=40)
            assert np.all(out.status == 0), out.status
            ends.append(out.y)
        fd = (ends[0] - ends[1]) / (2 * eps)
        for at, b in enumerate(rows):
            got = row_response(pa, p, ref.y, held, b, [picks[b][pick]], "level")[0]
            worst = max(worst, float(np.abs(got - fd[at]).max()))
    print("(%d, %d, %d): |level response - central difference| %.1e over %d rows" % (N, H, B, worst, len(rows)))
    assert worst <= 1e-6


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_every_reference_row_is_used_and_the_reductions_agree(N, H, B):
    import phoenix_amd as pa
    p, y0, held, ref = reference(N, H, B)
    free = moving(p, held, B)
    regs = sorted({k for b in range(B) for k in some_regulators(p, held, free, b)[1]})
    for input in ("level", "production"):
        rows = np.stack([row_response(pa, p, ref.y, held, b, regs, input) for b in range(B)])
        for reduce, want in (("mean", rows.mean(axis=0)), ("mean_abs", np.abs(rows).mean(axis=0))):
            out = pa.steady_state_response_reference(p, ref.y, clamp=held, regulators=regs, input=input, reduce=reduce)
            assert out.info.dtype == np.int32 and np.all(out.info == 0), out.info
            assert out.regulators == regs and np.abs(out.response - want).max() <= 1e-13
            mag = np.abs(out.response)
            mag[np.arange(len(regs)), regs] = 0
            assert np.allclose(out.scores, mag.sum(axis=1) / (N - 1), rtol=1e-13, atol=0)
    # rows that are left out: the mean divides by the rest
    if B >= 2:
        status = np.zeros(B, np.int32)
        status[0] = 1
        out = pa.steady_state_response_reference(p, ref.y, clamp=held, regulators=regs, status=status)
        rest = pa.steady_state_response_reference(p, ref.y[1:], clamp=held[1:], regulators=regs)
        # (not to the bit: numpy's products over the rows may take another order for another row count)
        assert out.info.tolist() == [-2] + [0] * (B - 1) and np.abs(out.response - rest.response).max() <= 1e-13


def test_a_singular_row_is_left_out_of_the_reference():
    import phoenix_amd as pa
    p, y = singular_model()
    out = pa.steady_state_response_reference(p, y, input="production", reduce="mean")
    assert out.info.tolist() == [0, 1, 0]
    rest = pa.steady_state_response_reference(p, y[[0, 2]], input="production", reduce="mean")
    assert np.abs(out.response - rest.response).max() <= 1e-13 and np.abs(out.response).max() > 0


# --------------------------------------------------------------------------- the C boundary and the Python caller
def test_the_symbols_are_exported_and_declared():
    from phoenix_amd import _lib as mod
    lib = mod.load()
    for name in NAMES:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    import phoenix_amd
    for name in ("steady_state_response", "steady_state_response_reference", "SteadyResponse"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.steady, name)
    assert phoenix_amd.SteadyResponse._fields == ("regulators", "response", "scores", "info")
    f = lib.phx_steady_inverse_workspace_bytes
    assert f.restype is C.c_size_t and f(3, 2) == 2 * 2 * 36 * 8 and f(0, 2) == f(257, 2) == f(3, 0) == 0


def test_bad_arguments_are_rejected_without_a_gpu():
    from phoenix_amd import _lib as mod
    lib = mod.load()
    good = dict(S=0xa000, H=3, B=2, Z=0xb000, info=0xf000, ws=0xe000, n=1 << 30)

    def inverse(**kw):
        a = dict(good, **kw)
        return lib.phx_steady_inverse(a["S"], a["H"], a["B"], a["Z"], a["info"], a["ws"], a["n"], None)
    for kw in (dict(S=None), dict(Z=None), dict(info=None), dict(H=0), dict(H=257), dict(B=0)):
        assert inverse(**kw) == BAD_ARG, kw
    assert inverse(ws=None) == WORKSPACE and inverse(n=2 * 2 * 36 * 8 - 1) == WORKSPACE
    addr = dict(Ws=0x1000, bs=0x2000, Wp=0x3000, bp=0x4000, WaT=0x5000, g=0x6000)

    def params(N=8, H=3, **null):
        a = dict(addr, **null)
        return mod.PhxParams(a["Ws"], a["bs"], a["Wp"], a["bp"], a["WaT"], a["g"], N, H, None)
    fgood = dict(p=params(), y=0x7000, m=0x8000, hid=0x9000, Z=0xa000, info=0xb000, B=2, genes=0xc000, K=5, input=1, X=0xd000,
                 use=0xe000)

    def factors(**kw):
        a = dict(fgood, **kw)
        return lib.phx_steady_response_factors(None if a["p"] is None else C.byref(a["p"]), a["y"], a["m"], a["hid"], a["Z"],
                                               a["info"], a["B"], a["genes"], a["K"], a["input"], a["X"], a["use"], None)
    for kw in [dict(p=None), dict(p=params(Ws=None)), dict(p=params(Wp=None)), dict(p=params(WaT=None)), dict(p=params(N=0)),
               dict(p=params(H=0)), dict(p=params(H=257)), dict(B=0), dict(B=65536), dict(K=0), dict(input=2), dict(input=-1)] + \
            [{k: None} for k in ("y", "m", "hid", "Z", "info", "genes", "X", "use")]:
        assert factors(**kw) == BAD_ARG, kw
    rgood = dict(p=params(), m=0x8000, X=0xd000, use=0xe000, B=2, genes=0xc000, K=5, input=1, mean_abs=1, out=0xf000, ld=8)

    def response(**kw):
        a = dict(rgood, **kw)
        return lib.phx_steady_response(None if a["p"] is None else C.byref(a["p"]), a["m"], a["X"], a["use"], a["B"], a["genes"],
                                       a["K"], a["input"], a["mean_abs"], a["out"], a["ld"], None)
    for kw in [dict(p=None), dict(p=params(WaT=None)), dict(p=params(N=0)), dict(p=params(H=257)), dict(B=0), dict(K=0),
               dict(input=2), dict(ld=7)] + [{k: None} for k in ("m", "X", "use", "genes", "out")]:
        assert response(**kw) == BAD_ARG, kw


def test_the_python_caller_checks_on_the_host_and_refuses_a_cpu_network():
    import phoenix_amd as pa
    net = pa.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    for kw in (dict(input="levels"), dict(input=1), dict(reduce="sum"), dict(reduce=None), dict(regulators=[16]),
               dict(regulators=[-1]), dict(regulators=[]), dict(rows_bytes=0), dict(rows_bytes=1.5), dict(status=torch.zeros(2)),
               dict(status=torch.zeros(3)), dict(status=torch.zeros(3, 1).long())):
        with pytest.raises(ValueError, match="steady_state_response"):
            pa.steady_state_response(net, y, **kw)
    with pytest.raises(TypeError, match="steady_state_response"):
        pa.steady_state_response(net, y, regulators=[0.5])
    for bad in (torch.rand(3, 15), torch.rand(16), torch.rand(3, 2, 16), torch.rand(3, 16).double(), torch.rand(0, 16), None):
        with pytest.raises(ValueError, match="steady_state_response"):
            pa.steady_state_response(net, bad)
    with pytest.raises((TypeError, ValueError), match="steady_state_response"):
        pa.steady_state_response(net, y, clamp=[0, 1])
    for kw in (dict(), dict(clamp=[0, -1, (1, 2)], regulators=[3, 1], input="production", reduce="mean", status=torch.zeros(3).int())):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            pa.steady_state_response(net, y, **kw)
    for kw in (dict(input="x"), dict(reduce="x"), dict(regulators=[16])):
        with pytest.raises(ValueError, match="steady_state_response_reference"):
            pa.steady_state_response_reference(net, y, **kw)
    out = pa.steady_state_response_reference(net, y, regulators=[2, 5])       # a module serves as `params` too
    assert out.response.shape == (2, 16) and out.scores.shape == (2,) and out.regulators == [2, 5]
