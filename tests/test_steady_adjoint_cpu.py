"""CPU-only checks of the implicit adjoint of the steady-state solve (phoenix_amd.steady_states(differentiable=True), DESIGN.md
section 8q): `steady_states_adjoint_reference`, the numpy restatement that tests/test_steady_adjoint_gpu.py holds the device
to, is pinned here to the adjoint of the dense N x N Jacobian with the explicit outer products and to central differences
through `steady_states_reference`; the exact zeros the formulas promise are exact; a row without a gradient contributes
nothing; the symbols exist and the argument checks answer before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols
from test_steady_cpu import C64, dense_jacobian, make_model, moving, parts64, reference

BAD_ARG, WORKSPACE = 4, 5
SHAPES = [(37, 5, 3), (97, 7, 5), (96, 56, 4), (70, 97, 3), (200, 200, 2)]
FIELDS = ("y0", "Ws", "bs", "Wp", "bp", "Wa", "g")


def cotangent(N, B):
    return np.random.default_rng(1000 + N).standard_normal((B, N))


def adjoint(N, H, B, **kw):
    import phoenix_amd
    p, y0, held, ref = reference(N, H, B)
    G = cotangent(N, B)
    return p, y0, held, ref, G, phoenix_amd.steady_states_adjoint_reference(p, ref.y, G, clamp=held, **kw)


# --------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_reference_equals_the_dense_adjoint(N, H, B):
    p, y0, held, ref, G, adj = adjoint(N, H, B)
    free = moving(p, held, B)
    q64 = {k: v.astype(np.float64) for k, v in p.items()}
    a, l, da, dl, hid, _ = parts64(p, ref.y)
    want = {"Ws": np.zeros((H, N)), "bs": np.zeros(H), "Wp": np.zeros((H, N)), "bp": np.zeros(H), "Wa": np.zeros((N, 2 * H)),
            "g": np.zeros(N), "y0": np.zeros((B, N))}
    lam = np.zeros((B, N))
    for b in range(B):
        f = free[b].astype(np.float64)
        # the N x N system: (I - P Wa C P)^T lam = P gy, and what the genes that do not move receive through C
        lam[b] = np.linalg.solve(dense_jacobian(p, ref.y, b, free[b]).T, f * G[b])
        Cb = C64(p, ref.y, b)
        z = q64["Wa"].T @ lam[b]                       # [2H]
        want["y0"][b] = (1 - f) * (G[b] + Cb.T @ z)
        want["Wa"] += np.outer(lam[b], hid[b])
        want["Ws"] += np.outer(z[:H], a[b])
        want["bs"] += z[:H]
        want["Wp"] += np.outer(z[H:] * hid[b, H:], l[b])
        want["bp"] += z[H:] * hid[b, H:]
    assert adj.info.dtype == np.int32 and np.all(adj.info == 0)
    scale = max(1.0, max(float(np.abs(v).max()) for v in want.values()))
    worst = {"lam": float(np.abs(adj.lam - lam).max())}
    for k in FIELDS:
        got = getattr(adj, k)
        assert got.shape == want[k].shape and got.dtype == np.float64, k
        worst[k] = float(np.abs(got - want[k]).max())
    print("(%d, %d, %d): largest gradient %.3g, |reference - dense adjoint| %s"
          % (N, H, B, scale, ", ".join("%s %.1e" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1e-9 * scale, worst


def _perturbed(p, y0, key, idx, h):
    p2 = {k: v.astype(np.float64).copy() for k, v in p.items()}
    y2 = y0.astype(np.float64).copy()
    (y2 if key == "y0" else p2[key])[idx] += h
    return p2, y2


@pytest.mark.parametrize("N,H,B", [(37, 5, 3), (97, 7, 5)])
def test_reference_equals_central_differences(N, H, B):
    """Central differences (h = 1e-6) of L = sum(y* G) through steady_states_reference(tol 1e-13, 60 steps): four entries of
    every parameter and six of y0, absolute agreement <= 1e-6.  Measured worst: 4.1e-9 at (37, 5, 3), 7.6e-9 at (97, 7, 5)."""
    import phoenix_amd
    p, y0, held, ref, G, adj = adjoint(N, H, B)
    free = moving(p, held, B)
    tight = phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-13, max_iter=60)
    assert np.all(tight.status == 0)
    adj = phoenix_amd.steady_states_adjoint_reference(p, tight.y, G, clamp=held)

    def loss(p2, y2):
        s = phoenix_amd.steady_states_reference(p2, y2, clamp=held, tol=1e-13, max_iter=60)
        assert np.all(s.status == 0)
        return float((s.y * G).sum())

    rng = np.random.default_rng(5)
    h, worst = 1e-6, 0.0
    for key in ("Ws", "Wp", "Wa", "bs", "bp", "g", "y0"):
        arr = y0 if key == "y0" else p[key]
        picks = [tuple(int(rng.integers(0, d)) for d in arr.shape) for _ in range(4)]
        if key == "y0":        # one held gene, one gene that never moves, and four at random
            picks = picks + [(b, held[b][0]) for b in range(B) if held[b]][:1] + [(0, int(np.nonzero(p["g"] <= 0)[0][0]))]
        if key == "g":         # entries of both signs away from 0
            picks = [(int(i),) for i in np.nonzero(p["g"] > 0)[0][:3]] + [(int(np.nonzero(p["g"] <= 0)[0][0]),)]
        for idx in picks:
            fd = (loss(*_perturbed(p, y0, key, idx, h)) - loss(*_perturbed(p, y0, key, idx, -h))) / (2 * h)
            got = float(getattr(adj, key)[idx])
            worst = max(worst, abs(fd - got))
            assert abs(fd - got) <= 1e-6, (key, idx, fd, got)
            if key == "y0" and free[idx]:
                assert got == 0.0
    print("(%d, %d, %d): |reference - central differences| <= %.1e" % (N, H, B, worst))


@pytest.mark.parametrize("N,H,B", [(37, 5, 3), (96, 56, 4)])
def test_exact_zero_structure(N, H, B):
    p, y0, held, ref, G, adj = adjoint(N, H, B)
    free = moving(p, held, B)
    assert not free.all() and any(held) and (p["g"] <= 0).any()
    assert np.all(adj.g == 0.0) and adj.g.shape == (N,)
    assert np.all(adj.y0[free] == 0.0) and np.all(adj.lam[~free] == 0.0)
    for b in range(B):
        want = G[b] + C64(p, ref.y, b).T @ adj.q[b]
        assert np.abs(adj.y0[b][~free[b]] - want[~free[b]]).max() <= 1e-12
        assert np.abs(adj.lam[b][free[b]] - want[free[b]]).max() <= 1e-12
        assert np.all(adj.y0[b][~free[b]] != 0.0)


def test_rows_without_a_gradient_contribute_exact_zeros():
    import phoenix_amd
    N, H, B = 97, 7, 5
    p, y0, held, ref = reference(N, H, B)
    G = cotangent(N, B)
    status = np.array([0, 1, 0, 2, 0], np.int32)
    got = phoenix_amd.steady_states_adjoint_reference(p, ref.y, G, clamp=held, status=status)
    G0 = np.where(status[:, None] == 0, G, 0.0)
    same = phoenix_amd.steady_states_adjoint_reference(p, ref.y, G0, clamp=held)
    assert got.info.tolist() == [0, -2, 0, -2, 0] and np.all(same.info == 0)
    for k in FIELDS + ("lam", "q"):
        assert np.array_equal(getattr(got, k), getattr(same, k)), k
    for b in (1, 3):
        assert np.all(got.y0[b] == 0.0) and np.all(got.lam[b] == 0.0) and np.all(got.q[b] == 0.0)
    # ... whatever the row holds: a state that is not finite
    y = ref.y.copy()
    y[1] = np.nan
    nan = phoenix_amd.steady_states_adjoint_reference(p, y, G, clamp=held, status=status)
    for k in FIELDS + ("lam", "q"):
        assert np.array_equal(getattr(nan, k), getattr(got, k)), k
    f32 = phoenix_amd.steady_states_adjoint_reference(p, ref.y, G0, clamp=held, dtype=np.float32)
    assert f32.Wa.dtype == np.float32 and np.abs(f32.Wa - same.Wa).max() < 1e-4 * max(1.0, np.abs(same.Wa).max())


def test_a_step_against_the_gradient_lowers_the_loss():
    import phoenix_amd
    for N, H, B in ((37, 5, 3), (97, 7, 5)):
        p, y0, held, ref, G, adj = adjoint(N, H, B)
        big = max(float(np.abs(getattr(adj, k)).max()) for k in FIELDS[1:])
        eps = 1e-3 / big
        p2 = {k: p[k].astype(np.float64) - eps * getattr(adj, k) for k in p}
        s = phoenix_amd.steady_states_reference(p2, y0, clamp=held, tol=1e-12, max_iter=40)
        assert np.all(s.status == 0)
        L0, L1 = float((ref.y * G).sum()), float((s.y * G).sum())
        first = -eps * sum(float((getattr(adj, k) ** 2).sum()) for k in FIELDS[1:])
        print("(%d, %d, %d): L %.6f -> %.6f, first order %.3e" % (N, H, B, L0, L1, first))
        assert L1 < L0


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


NAMES = ("phx_steady_adjoint_project", "phx_steady_adjoint_back", "phx_steady_param_grads",
         "phx_steady_adjoint_project_workspace_bytes", "phx_steady_param_grads_workspace_bytes")


def test_the_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in NAMES:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    import phoenix_amd
    for name in ("steady_states_adjoint_reference", "SteadyAdjoint", "last_backward_info"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.steady, name)
    assert phoenix_amd.SteadyAdjoint._fields == ("y0", "Ws", "bs", "Wp", "bp", "Wa", "g", "lam", "q", "info")
    for name in ("steady_adjoint_project", "steady_adjoint_back", "steady_param_grads"):
        assert callable(getattr(phoenix_amd.engine, name))
    assert phoenix_amd.last_backward_info() is None or phoenix_amd.last_backward_info().dtype == torch.int32


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _grads(mod, overwrite=1, **null):
    addr = {"Ws": 0x11000, "bs": 0x12000, "Wp": 0x13000, "bp": 0x14000, "WaT": None, "g": 0x16000, "Wa": 0x17000}
    addr.update(null)
    return mod.PhxGrads(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], overwrite, addr["Wa"])


def test_bad_arguments_are_rejected_without_a_gpu():
    """made-up device addresses: only calls that must return before touching the device"""
    mod, lib = _lib()
    shapes = (dict(N=0), dict(N=-8), dict(H=0), dict(H=257), dict(H=-1))

    def project(p="default", m=0x8000, gy=0x9000, B=3, b=0xb000, ws=0xe000, n=1 << 30):
        p = _params(mod) if p == "default" else p
        return lib.phx_steady_adjoint_project(None if p is None else C.byref(p), m, gy, B, b, ws, n, None)
    assert project(p=None) == BAD_ARG and project(p=_params(mod, WaT=None)) == BAD_ARG
    for kw in [dict(m=None), dict(gy=None), dict(b=None), dict(B=0), dict(B=-1)] + [dict(p=_params(mod, **s)) for s in shapes]:
        assert project(**kw) == BAD_ARG, kw
    need = lib.phx_steady_adjoint_project_workspace_bytes(8, 3, 3)
    assert need == 1 * 3 * 6 * 4
    assert project(ws=None) == WORKSPACE and project(n=need - 1) == WORKSPACE
    assert project(p=_params(mod, Ws=None, g=None), ws=None) == WORKSPACE       # Ws and g are not read

    def back(p="default", y=0x7000, m=0x8000, gy=0x9000, q=0xa000, hid=0xc000, B=3, lam=0xd000, gy0=0xf000):
        p = _params(mod) if p == "default" else p
        return lib.phx_steady_adjoint_back(None if p is None else C.byref(p), y, m, gy, q, hid, B, lam, gy0, None)
    assert back(p=None) == BAD_ARG and back(p=_params(mod, Ws=None)) == BAD_ARG and back(p=_params(mod, Wp=None)) == BAD_ARG
    for kw in [dict(y=None), dict(m=None), dict(gy=None), dict(q=None), dict(hid=None), dict(lam=None), dict(gy0=None), dict(B=0),
               dict(B=65536)] + [dict(p=_params(mod, **s)) for s in shapes]:
        assert back(**kw) == BAD_ARG, kw

    def pgrads(p="default", y=0x7000, lam=0xd000, q=0xa000, hid=0xc000, B=3, g="default", ws=0xe000, n=1 << 30):
        p = _params(mod) if p == "default" else p
        g = _grads(mod) if g == "default" else g
        return lib.phx_steady_param_grads(None if p is None else C.byref(p), y, lam, q, hid, B, None if g is None else C.byref(g),
                                          ws, n, None)
    assert pgrads(p=None) == BAD_ARG and pgrads(g=None) == BAD_ARG
    for kw in [dict(y=None), dict(lam=None), dict(q=None), dict(hid=None), dict(B=0), dict(B=-2)] + \
            [dict(p=_params(mod, **s)) for s in shapes] + \
            [dict(g=_grads(mod, **{k: None})) for k in ("Ws", "bs", "Wp", "bp", "Wa", "g")]:
        assert pgrads(**kw) == BAD_ARG, kw
    need = lib.phx_steady_param_grads_workspace_bytes(8, 3, 3)
    assert need == 1 * 12 * 9 * 4
    for kw in (dict(), dict(g=_grads(mod, overwrite=0, g=None)), dict(g=_grads(mod, WaT=0x15000, Wa=None)),
               dict(p=_params(mod, Ws=None, bs=None, Wp=None, bp=None, WaT=None, g=None))):      # no parameter is read
        assert pgrads(ws=None, **kw) == WORKSPACE, kw
    assert pgrads(n=need - 1) == WORKSPACE


def test_workspace_bytes():
    _, lib = _lib()
    f, g = lib.phx_steady_adjoint_project_workspace_bytes, lib.phx_steady_param_grads_workspace_bytes
    assert f.restype is C.c_size_t and g.restype is C.c_size_t
    for args in ((0, 40, 3), (-1, 40, 3), (350, 0, 3), (350, 257, 3), (350, 40, 0), (350, 40, -2)):
        assert f(*args) == 0 and g(*args) == 0, args
    # min(ceil(N / 32), 8) gene segments of [B][2H] floats
    assert f(33, 1, 1) == 2 * 1 * 2 * 4 and f(130, 40, 3) == 5 * 3 * 80 * 4 and f(11165, 40, 24) == 8 * 24 * 80 * 4
    # max(1, min(ceil(B / 32) / 2, ceil(512 / blocks))) row segments of [4H][N + 1] floats; blocks = ceil((N + 1) / 64) x
    # ceil((2 ceil(H / 16) + ceil(2H / 16)) / 4)
    assert g(33, 1, 1) == 4 * 34 * 4 and g(37, 5, 63) == g(37, 5, 95) == 20 * 38 * 4 and g(37, 5, 97) == g(37, 5, 131) == 2 * 20 * 38 * 4
    assert g(130, 40, 37) == 160 * 131 * 4 and g(97, 7, 70) == 28 * 98 * 4
    assert g(37, 5, 1 << 20) == 512 * 20 * 38 * 4
    assert g(11165, 40, 4096) == 1 * 160 * 11166 * 4              # 175 x 3 blocks: one pass over the rows fills the chip


# --------------------------------------------------------------------------- the Python callers
def test_the_differentiable_path_refuses_a_cpu_network_like_the_default_path():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16, requires_grad=True)
    for kw in (dict(), dict(clamp=[0, -1, (1, 2)]), dict(max_iter=3, return_reduced=True)):
        with pytest.raises(RuntimeError, match="must live on the GPU") as want:
            phoenix_amd.steady_states(net, y, **kw)
        with pytest.raises(RuntimeError, match="must live on the GPU") as got:
            phoenix_amd.steady_states(net, y, differentiable=True, **kw)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="steady_states"):
        phoenix_amd.steady_states(net, y, differentiable=True, tol=-1.0)
    with pytest.raises(ValueError, match="steady_states"):
        phoenix_amd.steady_states(net, torch.rand(3, 15), differentiable=True)
    with pytest.raises(ValueError, match="one shape"):
        phoenix_amd.steady_states_adjoint_reference(net, np.zeros((3, 16)), np.zeros((2, 16)))
