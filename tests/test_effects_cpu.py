"""CPU-only checks of the effects-matrix / state-Jacobian boundary (phx_effects_matrix / phx_effects_workspace_bytes,
include/phoenix_hip.h): the symbols exist, the argument checks answer before any device call, the Python callers refuse a
CPU network and bad arguments, and the fixture g20_effects.npz (tests/golden/make_golden_effects.py: the reference's own
effects matrix and autograd Jacobians) agrees with the closed forms of the header.

`closed_form` is the float64 evaluation of those formulas that tests/test_effects_gpu.py holds the kernel to."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
MODES = {"effects": 0, "mean": 1, "mean_abs": 2}
U = 2.0 ** -24


def act_grad64(y):
    """a', l' of include/phoenix_hip.h at float64(y)"""
    s = np.asarray(y, np.float64) - 0.5
    da = 1.0 / (1.0 + np.abs(s)) ** 2
    dl = np.where(s < 0, 1.0 / (1.0 + np.abs(s)), 1.0 / ((1.0 + s) * (1.0 + 2.0 * s)))
    return da, dl


def hidden64(p, y):
    """p[b, :] = exp(Wp log1p(softsign(y_b - 0.5)) + bp) in float64"""
    s = np.asarray(y, np.float64) - 0.5
    return np.exp(np.log1p(s / (1.0 + np.abs(s))) @ p["Wp"].astype(np.float64).T + p["bp"].astype(np.float64))


def closed_form(p, mode, y=None, ph=None, rows=None, per_state=False):
    """(ref, A) in float64 for regulator rows `rows` of parameters p (reference layouts: Ws, Wp [H, N], Wa [N, 2H], g [N]):
    ref = the formula of include/phoenix_hip.h on exactly these float32 inputs (ph included), A = the same formula with
    every factor and term replaced by its absolute value (delta kept).  per_state: the [B, R, N] Jacobians themselves."""
    H, N = p["Ws"].shape
    r0, r1 = (0, N) if rows is None else rows
    Ws, Wp = p["Ws"].astype(np.float64)[:, r0:r1], p["Wp"].astype(np.float64)[:, r0:r1]
    WaT = p["Wa"].astype(np.float64).T
    r = np.maximum(p["g"].astype(np.float64).reshape(-1), 0.0)
    S, aS = Ws.T @ WaT[:H], np.abs(Ws).T @ np.abs(WaT[:H])
    if mode == "effects":
        return r * (S + Wp.T @ WaT[H:]), r * (aS + np.abs(Wp).T @ np.abs(WaT[H:]))
    delta = np.zeros((r1 - r0, N))
    delta[np.arange(r1 - r0), np.arange(r0, r1)] = 1.0
    da, dl = act_grad64(y)
    ph = np.asarray(ph, np.float64)
    J, A = [], 0.0
    for b in range(len(y)):
        Q = (Wp * ph[b][:, None]).T @ WaT[H:]
        aQ = (np.abs(Wp) * np.abs(ph[b])[:, None]).T @ np.abs(WaT[H:])
        a, l = da[b, r0:r1, None], dl[b, r0:r1, None]
        J.append(r * (a * S + l * Q - delta))
        A = A + r * (np.abs(a) * aS + np.abs(l) * aQ + delta)
    J = np.stack(J)
    if per_state:
        return J, A / len(y)
    return (J.mean(0) if mode == "mean" else np.abs(J).mean(0)), A / len(y)


def kernel_bound(H, B, A):
    """|got - ref64| <= (2H + 16 + B) 2^-24 A[i, j]: 2H products and sums, at most 16 roundings in a', l', the scalings and
    the mean, B accumulations (B = 0 for the effects matrix); holds for any order of the sums"""
    return (2 * H + 16 + B) * U * A


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_effects_workspace_bytes", "phx_effects_matrix"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change
    assert mod.EFFECTS_MODES == MODES


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _call(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, row0=0, row1=8, out=0x9000, ws=None, ws_bytes=0):
    """phx_effects_matrix with made-up device addresses: only calls that must return before touching the device"""
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_matrix(None if p is None else C.byref(p), mode, y, ph, B, row0, row1, out, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    mod, lib = _lib()
    assert _call(mod, lib, p=None) == BAD_ARG
    assert _call(mod, lib, out=None) == BAD_ARG
    for name in ("Ws", "Wp", "WaT", "g"):
        assert _call(mod, lib, p=_params(mod, **{name: None})) == BAD_ARG, name
        assert _call(mod, lib, p=_params(mod, **{name: None}), mode=0) == BAD_ARG, name
    assert _call(mod, lib, p=_params(mod, N=1), row1=1) == BAD_ARG
    assert _call(mod, lib, p=_params(mod, H=0)) == BAD_ARG
    assert _call(mod, lib, p=_params(mod, H=257)) == BAD_ARG
    assert _call(mod, lib, p=_params(mod, N=-8)) == BAD_ARG
    assert _call(mod, lib, row0=-1) == BAD_ARG
    assert _call(mod, lib, row1=9) == BAD_ARG              # N = 8
    assert _call(mod, lib, row0=3, row1=3) == BAD_ARG
    assert _call(mod, lib, row0=5, row1=2) == BAD_ARG
    for mode in (-1, 3, 7):
        assert _call(mod, lib, mode=mode) == BAD_ARG, mode
    for mode in (1, 2):                                    # the Jacobian modes need their states
        assert _call(mod, lib, mode=mode, y=None) == BAD_ARG
        assert _call(mod, lib, mode=mode, ph=None) == BAD_ARG
        assert _call(mod, lib, mode=mode, B=0) == BAD_ARG
        assert _call(mod, lib, mode=mode, B=-2) == BAD_ARG
    # PHX_EFFECTS ignores y, ph and B -- but not its other arguments
    assert _call(mod, lib, mode=0, y=None, ph=None, B=0, row1=9) == BAD_ARG
    assert _call(mod, lib, mode=0, y=None, ph=None, B=0, out=None) == BAD_ARG


def test_workspace_bytes_is_zero_for_a_refused_shape():
    """no shape needs device scratch today: the function answers 0 for every shape, served or refused, so this test pins
    the contract (0 for a refused shape) for the day a shape does need scratch, and cannot fail before"""
    _, lib = _lib()
    f = lib.phx_effects_workspace_bytes
    for shape in ((1, 40, 3, 2), (0, 40, 3, 2), (-5, 40, 3, 2), (350, 0, 3, 2), (350, 257, 3, 2), (350, 40, 0, 2),
                  (350, 40, 3, 5), (350, 40, 3, -1)):
        assert f(*shape) == 0, shape
    assert f(350, 40, 3, 2) == f(350, 40, 3, 2)          # a plain function of the shape
    assert f.restype is C.c_size_t


def test_python_callers_have_no_cpu_path():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.effects_matrix(net)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.effects_matrix(net, rows=(3, 9))
    for reduce in ("mean", "mean_abs"):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.jacobian_matrix(net, torch.rand(3, 16), reduce=reduce)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.analysis.jacobian_matrix(net, torch.rand(3, 1, 16))


def test_bad_reduce_and_bad_rows_raise_value_errors():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    for reduce in ("sum", "abs", None, "effects", 1):
        with pytest.raises(ValueError, match="reduce"):
            phoenix_amd.jacobian_matrix(net, y, reduce=reduce)
    for rows in ((-1, 4), (0, 17), (5, 5), (9, 3), (3,), (1, 2, 3), 7, "ab"):
        with pytest.raises(ValueError, match="rows"):
            phoenix_amd.effects_matrix(net, rows=rows)
        with pytest.raises(ValueError, match="rows"):
            phoenix_amd.jacobian_matrix(net, y, rows=rows)


def test_golden_is_self_consistent():
    """g20: the reference's float32 effects matrix against the float64 formula of its own parameters, at the bar the
    kernel is held to; its float64 autograd Jacobians against the closed form; exact zeros where relu(g_j) = 0"""
    g = load_golden("g20_effects")
    p, y = sub(g, "p_"), g["y"]
    H, N = p["Ws"].shape
    assert (N, H) == (37, 5) and y.shape == (3, N) and y.dtype == np.float32 and g["effects"].dtype == np.float32
    assert g["jac64"].shape == g["jac32"].shape == (3, N, N)
    assert g["jac64"].dtype == np.float64 and g["jac32"].dtype == np.float32
    dead = p["g"] <= 0
    assert int(dead.sum()) >= 2 and int((y == 0.5).sum()) == 1 and (y < 0.5).any() and (y > 0.5).any()
    ref, A = closed_form(p, "effects")
    err = np.abs(g["effects"].astype(np.float64) - ref)
    bound = kernel_bound(H, 0, A)
    print("g20 effects vs float64 formula: worst |error| / bound = %.3f" % float(np.max(err[A > 0] / bound[A > 0])))
    assert np.all(err <= bound)
    J, _ = closed_form(p, "mean", y=y, ph=hidden64(p, y), per_state=True)
    e_j = float(np.max(np.abs(J - g["jac64"])))
    print("g20 jac64 vs closed form: max |difference| %.3e (max |jac64| %.3f)" % (e_j, float(np.max(np.abs(g["jac64"])))))
    assert e_j <= 1e-12
    assert np.all(g["effects"][:, dead] == 0) and np.all(g["jac64"][:, :, dead] == 0) and np.all(g["jac32"][:, :, dead] == 0)
    assert np.all(ref[:, dead] == 0) and np.all(J[:, :, dead] == 0)
