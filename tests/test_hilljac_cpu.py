"""The true Jacobian of the Hill-kinetics simulator and the recovery score against it, on the host: the sparsity pattern
of the shipped 350-gene network (golden G11), `simulator.jacobian_reference` -- the float64 yardstick of
tests/test_hilljac_gpu.py -- against central differences of Python's own evaluation of the expression strings, its float32
run against its float64 run (the room under the 5e-6 bar of the device), the signs against the `activation` flags of the
shipped edge table (golden G16), the derivative rules on hand-written systems, `analysis.recovery_scores`, and the
argument checks of phx_hill_jacobian, which need no device.

Metric of the Jacobian comparisons: |d| / max(1, |J64|), entry by entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_cpu import _declared_symbols

OK, BAD_ARG, WORKSPACE = 0, 4, 5
FD_H, FD_BAR = 1e-6, 1e-8        # central differences: truncation ~ h^2, rounding ~ eps / h = 2e-10
GPU_BAR = 5e-6                   # tests/test_hilljac_gpu.py: the project's bar for the simulator's rates
FP32_BAR = GPU_BAR / 4           # a float32 run of the same rules on the host must leave the device three quarters of it


def metric(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))


def rule_zeros(system, x):
    """bool [B, E]: the entries the derivative rules make exactly 0 at the states x, in any precision -- no path from the
    regulator to the rate that is not cut by an fAct at TF <= 0.  Interprets the programs on (value, "the derivative may be
    non-zero") pairs: PUSHC never, PUSHX of the regulator, the binary operators when either side may, fAct when TF > 0 and
    its argument may.  (A zero that the values produce by cancellation, such as d' - c d' at a c that rounds to 1, is not
    one of these, and a run in another precision need not repeat it.)"""
    x = np.asarray(x, np.float64)
    pat = system.jacobian_pattern()
    out = np.ones((x.shape[0], len(pat.regulator)), bool)
    for j in range(system.N):
        e0, e1 = pat.ptr[j], pat.ptr[j + 1]
        regs = pat.regulator[e0:e1]
        val, may = [], []
        for op, arg in system.code_host[system.off_host[j]: system.off_host[j] + system.len_host[j]].tolist():
            if op == 0:
                val.append(np.full(x.shape[0], system.consts_host[arg]))
                may.append(np.zeros((x.shape[0], len(regs)), bool))
            elif op == 1:
                val.append(x[:, arg])
                may.append(np.broadcast_to(regs == arg, (x.shape[0], len(regs))))
            elif op == 6:
                val[-1] = -val[-1]
            elif op == 7:
                b, k, n = system.consts_host[arg: arg + 3]
                may[-1] = may[-1] & (val[-1] > 0)[:, None]
                tn = np.where(val[-1] > 0, np.abs(val[-1]) ** n, 0.0)
                val[-1] = b * tn / (k + tn)
            else:
                r, rm = val.pop(), may.pop()
                val[-1] = val[-1] + r if op == 2 else val[-1] - r if op == 3 else val[-1] * r if op == 4 else val[-1] / r
                may[-1] = may[-1] | rm
        if e1 > e0:
            out[:, e0:e1] = ~may[0]
    return out


@functools.lru_cache(maxsize=None)
def g11_system():
    from phoenix_amd.simulator import HillSystem
    g = load_golden("g11_hill")
    names, eqns = [str(x) for x in g["names"]], [str(x) for x in g["eqns"]]
    return HillSystem(names, eqns, device="cpu"), names, eqns


def g11_states(B=6, seed=11):
    """float32 states from (1e-3, 1.2) with a tenth of the entries replaced by values from (-0.2, -1e-3)"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(1e-3, 1.2, (B, 350))
    neg = rs.rand(B, 350) < 0.1
    x[neg] = rs.uniform(-0.2, -1e-3, int(neg.sum()))
    return x.astype(np.float32)


def edge_flags():
    """{(regulator name, target name): activation} of the shipped edge_properties_G350.csv"""
    g = load_golden("g16_edges")
    return {(str(f), str(t)): str(a) == "TRUE" for f, t, a in zip(g["e350_from"], g["e350_to"], g["e350_activation"])}


# --------------------------------------------------------------------------- pattern
def test_pattern_of_the_shipped_network():
    sys_, _, _ = g11_system()
    pat = sys_.jacobian_pattern()
    assert pat is sys_.jacobian_pattern()                                        # cached
    for a in pat:
        assert isinstance(a, np.ndarray) and a.dtype == np.int64
    assert pat.regulator.shape == pat.target.shape == (823,) and pat.ptr.shape == (351,)
    diag = pat.regulator == pat.target
    assert int(diag.sum()) == 276 and int((~diag).sum()) == 547
    assert pat.ptr[0] == 0 and pat.ptr[-1] == 823 and np.all(np.diff(pat.ptr) >= 0) and int(np.diff(pat.ptr).max()) == 14
    assert int(sys_.len_host.max()) == 207
    for j in range(350):
        regs = pat.regulator[pat.ptr[j]:pat.ptr[j + 1]]
        assert np.all(pat.target[pat.ptr[j]:pat.ptr[j + 1]] == j)
        assert np.all(np.diff(regs) > 0)                                         # ascending, distinct
        if sys_.is_input[j]:
            assert len(regs) == 0
        else:
            prog = sys_.code_host[sys_.off_host[j]: sys_.off_host[j] + sys_.len_host[j]]
            assert set(regs.tolist()) == set(prog[prog[:, 0] == 1, 1].tolist()) and j in regs
    assert np.array_equal(np.flatnonzero(np.diff(pat.ptr) == 0), np.flatnonzero(sys_.is_input))


# --------------------------------------------------------------------------- the yardstick
def test_reference_against_central_differences():
    from oracle import hill_oracle
    from phoenix_amd.simulator import jacobian_reference
    sys_, names, eqns = g11_system()
    pat = sys_.jacobian_pattern()
    x = g11_states().astype(np.float64)
    assert np.all(np.abs(x) > 1e-3 - 1e-9) and 0.05 < np.mean(x < 0) < 0.15 and x.max() > 1
    J = jacobian_reference(sys_, x)
    assert J.shape == (6, 823) and J.dtype == np.float64 and np.all(np.isfinite(J))
    f = hill_oracle.compile_rhs(names, eqns, hill_oracle.fAct0)
    regs = np.unique(pat.regulator)
    xb = np.broadcast_to(x, (len(regs), 2, 6, 350)).copy()
    xb[np.arange(len(regs)), 0, :, regs] += FD_H
    xb[np.arange(len(regs)), 1, :, regs] -= FD_H
    out = f(xb)                                                                  # [regs, +-, 6, 350]
    at = np.searchsorted(regs, pat.regulator)
    fd = (out[at, 0, :, pat.target] - out[at, 1, :, pat.target]).T / (2 * FD_H)  # [6, 823]
    err = metric(J, fd)
    print("fp64 reference against central differences: %.2e (entry %d)" % (err.max(), int(err.max(axis=0).argmax())))
    assert err.max() < FD_BAR
    assert np.count_nonzero(J) > 0.8 * J.size and np.any(J == 0)                 # negative regulators: exact zeros


def test_float32_run_of_the_reference_leaves_the_device_room():
    from phoenix_amd.simulator import jacobian_reference
    sys_, _, _ = g11_system()
    x = g11_states()
    J64 = jacobian_reference(sys_, x.astype(np.float64))
    J32 = jacobian_reference(sys_, x, dtype=np.float32)
    assert J32.dtype == np.float32 and J32.shape == J64.shape
    err = metric(J32, J64)
    print("fp32 run against the fp64 run: %.2e" % err.max())
    assert err.max() < FP32_BAR
    zero = rule_zeros(sys_, x)
    assert np.all(J32[zero] == 0) and np.all(J64[zero] == 0) and 0.05 < zero.mean() < 0.2    # 0 in any precision

def test_signs_are_the_activation_flags_of_the_edge_table():
    from phoenix_amd.simulator import jacobian_reference
    sys_, names, _ = g11_system()
    pat = sys_.jacobian_pattern()
    flags = edge_flags()
    assert len(flags) == 550
    x = np.random.RandomState(16).uniform(0.05, 1.0, (8, 350))
    J = jacobian_reference(sys_, x)
    seen = set()
    for e, (r, t) in enumerate(zip(pat.regulator.tolist(), pat.target.tolist())):
        if r == t:
            assert np.all(J[:, e] < 0), names[t]                                 # the decay term
            continue
        key = (names[r], names[t])
        assert key in flags, key
        seen.add(key)
        assert np.all(J[:, e] > 0) if flags[key] else np.all(J[:, e] < 0), key
    assert len(seen) == 547                                                      # 3 shipped edges are in no expression


# --------------------------------------------------------------------------- the rules, on hand-written systems
def _tiny(expr):
    from phoenix_amd.simulator import HillSystem
    return HillSystem(["a", "b", "y"], ["input gene", "input gene", expr], device="cpu")


def test_derivative_rules_in_closed_form():
    from phoenix_amd.simulator import HillPattern, fact_constants, jacobian_reference
    x = np.array([[0.3, 0.7, 0.2], [1.1, -0.15, 0.9], [-0.05, 0.4, 0.6], [0.0, 0.25, -0.1]])
    a, b = x[:, 0], x[:, 1]
    # a / (1 + b): q = a / (1 + b), d/da = 1 / (1 + b), d/db = -q / (1 + b)
    s = _tiny("a / (1 + b)")
    assert s.jacobian_pattern().regulator.tolist() == [0, 1] and s.jacobian_pattern().ptr.tolist() == [0, 0, 0, 2]
    J = jacobian_reference(s, x)
    assert np.array_equal(J[:, 0], 1.0 / (1 + b)) and np.array_equal(J[:, 1], (0.0 - a / (1 + b)) / (1 + b))
    # -(a * b)
    J = jacobian_reference(_tiny("-(a * b)"), x)
    assert np.array_equal(J[:, 0], -b) and np.array_equal(J[:, 1], -a)
    # a variable that occurs twice, and the self entry
    s = _tiny("a * a + a - 0.5 * y")
    assert s.jacobian_pattern().regulator.tolist() == [0, 2]
    J = jacobian_reference(s, x)
    assert np.array_equal(J[:, 0], (a + a) + 1) and np.array_equal(J[:, 1], np.full(4, -0.5))
    # fAct: B K n tf^(n-1) / (K + tf^n)^2 for tf > 0; exactly 0 at tf = 0 and tf < 0
    s = _tiny("0.8 * fAct(a, 0.4, 2.5) - y")
    Bc, K, n = fact_constants(0.4, 2.5)
    J = jacobian_reference(s, x)
    want = np.zeros(4)
    pos = a > 0
    want[pos] = 0.8 * (Bc * K * n * a[pos] ** (n - 1) / (K + a[pos] ** n) ** 2)
    assert np.max(np.abs(J[:, 0] - want)) < 1e-15 and np.all(J[~pos, 0] == 0) and int((~pos).sum()) == 2
    assert np.all(want[pos] > 0) and np.array_equal(J[:, 1], np.full(4, -1.0))
    # ... and the chain rule through an inner expression: fAct(a * b) at a b <= 0 is flat
    J = jacobian_reference(_tiny("fAct(a * b, 0.4, 2.0) - y"), x)
    tf = a * b
    B2, K2, _ = fact_constants(0.4, 2.0)
    inner = np.where(tf > 0, B2 * K2 * 2.0 * np.abs(tf) / (K2 + tf ** 2) ** 2, 0.0)
    assert np.max(np.abs(J[:, 0] - inner * b)) < 1e-14 and np.max(np.abs(J[:, 1] - inner * a)) < 1e-14
    assert np.all(J[tf <= 0, :2] == 0) and np.any(tf <= 0) and np.any(tf > 0)
    # an entry whose regulator the program never pushes: +0, not the -0 the rules would leave behind a NEG
    s = _tiny("-(a * a)")
    pat = HillPattern(np.array([0, 1], np.int64), np.array([2, 2], np.int64), np.array([0, 0, 0, 2], np.int64))
    for dt in (np.float64, np.float32):
        J = jacobian_reference(s, x, dtype=dt, pattern=pat)
        assert np.all(J[:, 1] == 0) and not np.any(np.signbit(J[:, 1]))
        assert np.array_equal(J[:, 0], -(a.astype(dt) + a.astype(dt))) and J.dtype == dt


def test_reference_takes_both_state_shapes_and_refuses_others():
    from phoenix_amd.simulator import jacobian_reference
    s = _tiny("a / (1 + b) - y")
    x = np.random.RandomState(3).uniform(0.1, 1, (5, 3))
    assert np.array_equal(jacobian_reference(s, x), jacobian_reference(s, x.reshape(5, 1, 3)))
    for bad in (x[:, :2], x.reshape(1, 5, 3), x[0], x[:0]):
        with pytest.raises(ValueError, match="x must be"):
            jacobian_reference(s, bad)


# --------------------------------------------------------------------------- recovery_scores
def test_recovery_scores():
    from phoenix_amd import recovery_scores
    rs = np.random.RandomState(5)
    t = rs.randn(40)
    assert recovery_scores(t, t) == (1.0, 1.0, 1.0, 1.0)
    assert recovery_scores(t, -t) == (0.0, -1.0, -1.0, -1.0)
    assert recovery_scores(t.astype(np.float32), 4 * t.astype(np.float32)) == (1.0, 1.0, 1.0, 4.0)
    # average ranks: t = (1, 2, 2, 3) ranks (1, 2.5, 2.5, 4); against (1, 2, 3, 4): 4.5 / sqrt(4.5 * 5)
    sign, pearson, spearman, slope = recovery_scores([1.0, 2.0, 2.0, 3.0], [10.0, 20.0, 30.0, 45.0])
    assert sign == 1.0 and abs(spearman - 4.5 / np.sqrt(22.5)) < 1e-15 and spearman < pearson < 1
    assert abs(slope - (10 + 40 + 60 + 135) / 18.0) < 1e-14
    # signs: a learned 0 disagrees, entries with true == 0 do not count
    assert recovery_scores([1.0, -2.0, 0.0, 3.0, -1.0], [0.5, 0.0, 7.0, -1.0, -2.0])[0] == 2 / 4
    # undefined statistics are NaN, not exceptions
    sign, pearson, spearman, slope = recovery_scores([2.0], [3.0])
    assert sign == 1.0 and np.isnan(pearson) and np.isnan(spearman) and slope == 1.5
    sign, pearson, spearman, slope = recovery_scores([2.0, 2.0, 2.0], [1.0, 2.0, 3.0])
    assert sign == 1.0 and np.isnan(pearson) and np.isnan(spearman) and slope == 1.0
    assert np.isnan(recovery_scores([1.0, 2.0, 3.0], [4.0, 4.0, 4.0])[1])
    assert all(np.isnan(v) for v in recovery_scores([], []))
    assert all(np.isnan(v) for v in recovery_scores([0.0, 0.0], [1.0, 2.0]))
    with pytest.raises(ValueError, match="same length"):
        recovery_scores([1.0, 2.0], [1.0])


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_hill_jacobian_workspace_bytes", "phx_hill_jacobian"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    import phoenix_amd
    for name in ("jacobian_recovery", "recovery_scores", "JacobianRecovery"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.analysis, name), name
    for name in ("HillPattern", "HillJacobian", "jacobian_reference"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.simulator, name), name
    from phoenix_amd import build
    assert any(s.endswith("phx_hilljac.hip") for s in build.sources())


def _call(lib, code=0x1000, off=0x2000, len_=0x3000, consts=0x4000, eptr=0x5000, ereg=0x6000, x=0x7000, B=6, N=350, E=823,
          mode=0, out=0x8000, ws=0x9000, ws_bytes=1 << 40):
    """phx_hill_jacobian with made-up device addresses: only calls that must return before touching the device"""
    return lib.phx_hill_jacobian(code, off, len_, consts, eptr, ereg, x, B, N, E, mode, out, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    _, lib = _lib()
    for bad in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-7), dict(E=-1), dict(E=-2 ** 40), dict(mode=-1), dict(mode=3)):
        for mode in (0, 1, 2):
            assert _call(lib, **dict(dict(mode=mode), **bad)) == BAD_ARG, bad
    for name in ("code", "off", "len_", "consts", "eptr", "ereg", "x", "out"):
        for E in (823, 0):
            assert _call(lib, E=E, **{name: None}) == BAD_ARG, name
    # an empty pattern is served, with nothing launched
    for mode in (0, 1, 2):
        assert _call(lib, E=0, mode=mode, ws=None, ws_bytes=0) == OK
        assert _call(lib, E=0, mode=mode, B=4099, ws=None, ws_bytes=0) == OK
    # the chunk sums of the reduced modes
    need = lib.phx_hill_jacobian_workspace_bytes(257, 350, 823, 1)
    assert need > 0
    for mode in (1, 2):
        assert _call(lib, B=257, mode=mode, ws=None) == WORKSPACE
        assert _call(lib, B=257, mode=mode, ws_bytes=need - 1) == WORKSPACE
        assert _call(lib, B=289, mode=mode, ws_bytes=need) == WORKSPACE       # one more chunk


def test_workspace_bytes():
    _, lib = _lib()
    f = lib.phx_hill_jacobian_workspace_bytes
    assert f.restype is C.c_size_t
    for args in ((0, 350, 823, 1), (257, 0, 823, 1), (257, 350, -1, 2), (257, 350, 823, 3), (257, 350, 823, -1)):
        assert f(*args) == 0, args
    for B in (1, 32, 257, 10 ** 6):
        assert f(B, 350, 823, 0) == 0                                            # mode 0 needs none
    for mode in (1, 2):
        # min(1024, ceil(B / 32)) chunks of E doubles; one chunk is written straight to the result
        for B, S in ((1, 0), (2, 0), (32, 0), (33, 2), (257, 9), (4099, 129), (32768, 1024), (10 ** 6, 1024)):
            assert f(B, 350, 823, mode) == S * 823 * 8, (B, mode)
        assert f(257, 350, 0, mode) == 0 and f(257, 1, 2 ** 33, mode) == 9 * 2 ** 36 and f(257, 7, 823, mode) == f(257, 350, 823, mode)


# --------------------------------------------------------------------------- the Python callers
def test_python_callers_refuse_what_they_cannot_serve():
    import phoenix_amd
    sys_, _, _ = g11_system()
    x = torch.rand(3, 350)
    for kw in (dict(), dict(reduce="mean"), dict(reduce="mean_abs")):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            sys_.jacobian(x, **kw)
    for reduce in ("sum", "abs", 0, "effects"):
        with pytest.raises(ValueError, match="reduce"):
            sys_.jacobian(x, reduce=reduce)
    with pytest.raises(TypeError, match="tensor"):
        sys_.jacobian(x.numpy())
    # a model of another gene count: refused before a device is needed
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    for diagonal in (False, True):
        with pytest.raises(ValueError, match="16 genes, the system 350"):
            phoenix_amd.jacobian_recovery(net, sys_, x, diagonal=diagonal)
    net = phoenix_amd.ODENet("cpu", 350, neurons=4)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.jacobian_recovery(net, sys_, x)
