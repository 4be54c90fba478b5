"""CPU-only checks of the steady-state solve (phoenix_amd.steady_states and its kernel's C boundary, phx_reduced_jacobian /
phx_steady_*, include/phoenix_hip.h): `steady_states_reference`, the numpy restatement that tests/test_steady_gpu.py holds
the device iteration to, converges on every test model and is pinned here to a brute-force Newton on the dense N x N
Jacobian; the Woodbury form of the step equals the dense linearly implicit step; the symbols exist and the argument checks
answer before any device call.  The test models and the float64 formulas of the GPU tests live here too."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
# (N, H, B): the smallest shapes that cross the 16-wide tiles, the 64-wide blocks, the 32-gene chunks and, in the last four,
# lie on either side of the first gene count at which a segment holds two chunks (N = 32 S + 1; S = 5 at H = 200, 16 at 97)
SHAPES = [(33, 1, 1), (37, 5, 3), (97, 7, 5), (96, 44, 5), (96, 56, 4), (130, 40, 3), (70, 97, 3), (200, 200, 2), (350, 30, 7),
          (1100, 48, 6), (160, 200, 1), (161, 200, 1), (512, 97, 2), (513, 97, 2)]


def make_model(N, H, B, g_lo=0.2, g_hi=1.2):
    """(params dict of float32 arrays in the reference layouts, y0 [B, N] float32, held sets): Ws, Wp ~ N(0, (c1 / sqrt N)^2),
    Wa ~ N(0, (c2 / sqrt 2H)^2), biases U(-0.1, 0.1), g ~ U(g_lo, g_hi) with max(1, N // 16) entries negated (genes that
    never move), (c1, c2) = (1.5, 0.6) for H <= 56 and (1.0, 0.45) above; y0 ~ U[0, 1); held sets of sizes 0 .. 4 cycle"""
    c1, c2 = (1.5, 0.6) if H <= 56 else (1.0, 0.45)
    r = np.random.default_rng(N + H)
    p = {"Ws": r.normal(0, c1 / np.sqrt(N), (H, N)), "Wp": r.normal(0, c1 / np.sqrt(N), (H, N)),
         "Wa": r.normal(0, c2 / np.sqrt(2 * H), (N, 2 * H)), "bs": r.uniform(-.1, .1, H), "bp": r.uniform(-.1, .1, H),
         "g": r.uniform(g_lo, g_hi, N)}
    p["g"][r.choice(N, max(1, N // 16), replace=False)] *= -1
    p = {k: v.astype(np.float32) for k, v in p.items()}
    r = np.random.default_rng(N)
    y0 = r.random((B, N)).astype(np.float32)
    held = [tuple(int(k) for k in r.choice(N, b % 5, replace=False)) for b in range(B)]
    return p, y0, held


def moving(p, held, B):
    free = np.repeat((p["g"] > 0)[None, :], B, axis=0)
    for b, s in enumerate(held):
        free[b, list(s)] = False
    return free


def parts64(p, y):
    """float64: a, l, a', l', the hidden vector hid [B, 2H] and r = Wa hid - y of the states y [B, N]"""
    q = {k: v.astype(np.float64) for k, v in p.items()}
    y = np.asarray(y, np.float64)
    s = y - 0.5
    d = 1 + np.abs(s)
    a = s / d
    l = np.log1p(a)
    da = 1 / (d * d)
    dl = da / (1 + a)
    hid = np.concatenate([a @ q["Ws"].T + q["bs"], np.exp(l @ q["Wp"].T + q["bp"])], axis=1)
    return a, l, da, dl, hid, hid @ q["Wa"].T - y


def C64(p, y, b):
    """C(y_b) [2H, N] in float64"""
    _, _, da, dl, hid, _ = parts64(p, y)
    H = p["Ws"].shape[0]
    return np.concatenate([p["Ws"].astype(np.float64) * da[b][None, :],
                           hid[b, H:, None] * p["Wp"].astype(np.float64) * dl[b][None, :]], axis=0)


def dense_jacobian(p, y, b, free_b):
    """I - diag(free) Wa C diag(free), N x N float64"""
    f = free_b.astype(np.float64)
    return np.eye(len(f)) - f[:, None] * (p["Wa"].astype(np.float64) @ C64(p, y, b)) * f[None, :]


def rho64(p, y, free):
    return np.where(free, np.abs(parts64(p, y)[5]), 0).max(axis=1)


_REF = {}


def reference(N, H, B):
    """(p, y0, held, steady_states_reference(float64, tol 1e-12, 40 steps)) of a test shape, computed once"""
    if (N, H, B) not in _REF:
        import phoenix_amd
        p, y0, held = make_model(N, H, B)
        _REF[(N, H, B)] = (p, y0, held, phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=40))
    return _REF[(N, H, B)]


# --------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("N,H,B", SHAPES)
def test_reference_converges_on_every_row_and_equals_a_dense_newton(N, H, B):
    p, y0, held, ref = reference(N, H, B)
    free = moving(p, held, B)
    assert ref.y.dtype == np.float64 and ref.y.shape == (B, N) and ref.status.dtype == np.int32
    assert np.all(ref.status == 0), ref.status                 # none is left out: the GPU comparisons are not vacuous
    assert np.all(ref.iterations <= 40) and np.all(ref.iterations >= 1), ref.iterations
    assert np.all(ref.residual <= 1e-12) and np.array_equal(ref.residual, rho64(p, ref.y, free))
    assert np.array_equal(ref.y[~free], y0.astype(np.float64)[~free])       # held genes and genes with g <= 0: to the bit
    # brute-force Newton on the dense Jacobian, started from the reference's result
    y = ref.y.copy()
    for _ in range(3):
        r = parts64(p, y)[5]
        for b in range(B):
            y[b] += np.linalg.solve(dense_jacobian(p, y, b, free[b]), np.where(free[b], r[b], 0))
    rad = max(float(np.abs(np.linalg.eigvals(ref.reduced[b])).max()) for b in range(B))
    print("(%d, %d, %d): steps %s, residual %.1e, |dense Newton - reference| %.1e, spectral radius of S up to %.2f"
          % (N, H, B, ref.iterations.tolist(), ref.residual.max(), np.abs(y - ref.y).max(), rad))
    assert np.abs(y - ref.y).max() <= 1e-10
    assert rho64(p, y, free).max() <= 1e-12
    # reduced: S with unit weights on the moving genes at the result
    for b in range(B):
        assert np.allclose(ref.reduced[b], (C64(p, ref.y, b) * free[b][None, :]) @ p["Wa"].astype(np.float64), rtol=0, atol=1e-12)


@pytest.mark.parametrize("tau", [0.5, 10.0, float("inf")])
def test_the_woodbury_step_equals_the_dense_linearly_implicit_step(tau):
    import phoenix_amd
    worst = 0.0
    for N, H, B in ((37, 5, 3), (96, 44, 5), (70, 97, 3)):
        p, y0, held, ref = reference(N, H, B)
        free = moving(p, held, B)
        rng = np.random.default_rng(7)
        start = ref.y + np.where(free, 1e-3 * rng.standard_normal((B, N)), 0)       # near enough that every step is accepted
        one = phoenix_amd.steady_states_reference(p, start, clamp=held, tol=1e-12, max_iter=1, tau0=tau)
        assert np.all(one.iterations == 1) and np.all(one.residual < rho64(p, start, free))
        gp = np.maximum(p["g"].astype(np.float64), 0)
        r = parts64(p, start)[5]
        for b in range(B):
            m = np.where(free[b], 1.0 if np.isinf(tau) else tau * gp / (1 + tau * gp), 0.0)
            # (I - tau J) delta = tau f with J = diag(g+) (Wa C - I) on the moving genes, divided by I + tau diag(g+)
            dense = np.linalg.solve(np.eye(N) - m[:, None] * (p["Wa"].astype(np.float64) @ C64(p, start, b)), m * r[b])
            worst = max(worst, float(np.abs(one.y[b] - start[b] - dense).max()))
    print("tau %g: |Woodbury step - dense step| %.1e" % (tau, worst))
    assert worst <= 1e-10


def test_reference_control():
    import phoenix_amd
    p, y0, held, ref = reference(97, 7, 5)
    two = phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=2)
    assert np.all(two.status == 1) and np.all(two.iterations == 2)
    none = phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-12, max_iter=0)
    assert np.array_equal(none.y, y0.astype(np.float64)) and np.all(none.iterations == 0) and np.all(none.status == 1)
    f32 = phoenix_amd.steady_states_reference(p, y0, clamp=held, tol=1e-5, max_iter=40, dtype=np.float32)
    assert f32.y.dtype == np.float32 and np.all(f32.status == 0) and np.abs(f32.y - ref.y).max() < 1e-3
    net = phoenix_amd.ODENet("cpu", 97, neurons=7)             # a module serves as `params` too
    got = phoenix_amd.steady_states_reference(net, y0, max_iter=3)
    assert got.y.shape == (5, 97)


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


NAMES = ("phx_reduced_jacobian_workspace_bytes", "phx_reduced_jacobian", "phx_steady_residual", "phx_steady_update",
         "phx_steady_solve_workspace_bytes", "phx_steady_solve")


def test_the_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in NAMES:
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    import phoenix_amd
    for name in ("steady_states", "steady_states_reference", "reduced_jacobian", "knockout_steady_states", "SteadyStates",
                 "KnockoutSteadyStates"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.steady, name)
    assert phoenix_amd.SteadyStates._fields == ("y", "residual", "iterations", "status", "tau", "reduced")


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _call(mod, lib, p="default", y=0x7000, m=0x8000, r=0x9000, B=3, S=0xa000, w=0xb000, hid=0xc000, ws=0xe000, ws_bytes=1 << 30):
    """phx_reduced_jacobian with made-up device addresses: only calls that must return before touching the device"""
    if p == "default":
        p = _params(mod)
    return lib.phx_reduced_jacobian(None if p is None else C.byref(p), y, m, r, B, S, w, hid, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    mod, lib = _lib()
    assert _call(mod, lib, p=None) == BAD_ARG
    for name in ("Ws", "bs", "Wp", "bp", "WaT"):
        assert _call(mod, lib, p=_params(mod, **{name: None})) == BAD_ARG, name
    for bad in (dict(N=0), dict(N=-8), dict(H=0), dict(H=257), dict(H=-1)):
        assert _call(mod, lib, p=_params(mod, **bad)) == BAD_ARG, bad
    for name in ("y", "m", "S", "hid"):
        assert _call(mod, lib, **{name: None}) == BAD_ARG, name
    assert _call(mod, lib, r=None) == BAD_ARG and _call(mod, lib, w=None) == BAD_ARG      # w goes with r
    for B in (0, -1):
        assert _call(mod, lib, B=B) == BAD_ARG
    # every argument in order: the workspace is asked for next (g is not read: a null g passes)
    need = lib.phx_reduced_jacobian_workspace_bytes(8, 3, 3)
    assert need > 0
    for kw in (dict(), dict(r=None, w=None), dict(p=_params(mod, g=None)), dict(p=_params(mod, N=1, H=256))):
        assert _call(mod, lib, ws=None, **kw) == WORKSPACE, kw
    assert _call(mod, lib, ws_bytes=need - 1) == WORKSPACE
    # the passes of the iteration
    p = _params(mod)
    assert lib.phx_steady_residual(None, 0x7000, 3, 0xc000, 0x9000, None) == BAD_ARG
    for args in ((None, 3, 0xc000, 0x9000), (0x7000, 0, 0xc000, 0x9000), (0x7000, 65536, 0xc000, 0x9000), (0x7000, 3, None, 0x9000),
                 (0x7000, 3, 0xc000, None)):
        assert lib.phx_steady_residual(C.byref(p), *args, None) == BAD_ARG, args
    assert lib.phx_steady_residual(C.byref(_params(mod, H=257)), 0x7000, 3, 0xc000, 0x9000, None) == BAD_ARG
    good = [0x7000, 0x8000, 0x9000, 0xd000, 3, 0xf000]
    assert lib.phx_steady_update(None, *good, None) == BAD_ARG
    for at in range(6):
        args = list(good)
        args[at] = 0 if at == 4 else None
        assert lib.phx_steady_update(C.byref(p), *args, None) == BAD_ARG, at
    assert lib.phx_steady_update(C.byref(_params(mod, WaT=None)), *good, None) == BAD_ARG
    sgood = dict(S=0xa000, w=0xb000, H=3, B=2, x=0xd000, info=0xf000, ws=0xe000, n=1 << 30)

    def solve(**kw):
        a = dict(sgood, **kw)
        return lib.phx_steady_solve(a["S"], a["w"], a["H"], a["B"], a["x"], a["info"], a["ws"], a["n"], None)
    for kw in (dict(S=None), dict(w=None), dict(x=None), dict(info=None), dict(H=0), dict(H=257), dict(B=0)):
        assert solve(**kw) == BAD_ARG, kw
    assert solve(ws=None) == WORKSPACE and solve(n=2 * 36 * 8 - 1) == WORKSPACE


def test_workspace_bytes():
    _, lib = _lib()
    f = lib.phx_reduced_jacobian_workspace_bytes
    assert f.restype is C.c_size_t
    for args in ((0, 40, 3), (-1, 40, 3), (350, 0, 3), (350, 257, 3), (350, 40, 0), (350, 40, -2)):
        assert f(*args) == 0, args
    # S partial blocks [B][2H][2H + 2] floats; S = min(ceil(N / 32), ceil(256 / (2 ceil(H / 64) ceil((2H + 2) / 64))))
    assert f(33, 1, 1) == 2 * 1 * 2 * 4 * 4
    assert f(130, 40, 3) == 5 * 3 * 80 * 82 * 4
    assert f(160, 200, 1) == f(161, 200, 1) == 5 * 400 * 402 * 4              # 5 chunks in 5 segments, 6 chunks in 5
    assert f(11165, 40, 24) == 64 * 24 * 80 * 82 * 4
    # more states than 64 MiB of partial blocks hold are walked in chunks of a multiple of four
    assert f(11165, 40, 60) == 36 * 64 * 80 * 82 * 4 <= 64 << 20 < 40 * 64 * 80 * 82 * 4
    per = 5 * 400 * 402 * 4
    chunk = (64 << 20) // per // 4 * 4
    assert f(14691, 200, 24) == chunk * per and 4 <= chunk < 24
    assert f(14691, 200, chunk) == f(14691, 200, 1 << 20) == chunk * per and f(14691, 200, 3) == 3 * per
    g = lib.phx_steady_solve_workspace_bytes
    assert g.restype is C.c_size_t and g(3, 2) == 2 * 36 * 8 and g(0, 2) == g(257, 2) == g(3, 0) == 0


# --------------------------------------------------------------------------- the Python callers
def test_python_callers_check_on_the_host_and_refuse_a_cpu_network():
    import phoenix_amd
    from phoenix_amd.odeint import _clamp_list
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    # clamp errors are _clamp_list's, raised before a device is asked for
    for bad in ([0, 1], [0, 1, 16], [0, -2, 1], [(0, 1, 2, 3, 4), 1, 2], [0.5, 1, 2], torch.zeros(3), torch.zeros(3, 2, 2).long(), 5):
        with pytest.raises((TypeError, ValueError)) as want:
            _clamp_list(bad, 3, 16, who="steady_states", unit="row")
        with pytest.raises(type(want.value)) as got:
            phoenix_amd.steady_states(net, y, clamp=bad)
        assert str(got.value) == str(want.value)
        with pytest.raises(type(want.value), match="reduced_jacobian"):
            phoenix_amd.reduced_jacobian(net, y, clamp=bad)
    for kw in (dict(tol=-1e-6), dict(tol="1e-5"), dict(tol=float("nan")), dict(tol=float("inf")), dict(max_iter=-1),
               dict(max_iter=2.5), dict(max_iter=True), dict(tau0=0.0), dict(tau0=-1.0), dict(tau0=float("nan")), dict(tau0="1")):
        with pytest.raises(ValueError, match="steady_states"):
            phoenix_amd.steady_states(net, y, **kw)
        with pytest.raises(ValueError, match="steady_states_reference"):
            phoenix_amd.steady_states_reference(net, y, **kw)
    for bad in (torch.rand(3, 15), torch.rand(16), torch.rand(3, 2, 16), torch.rand(3, 16).double(), torch.rand(0, 16), None):
        with pytest.raises(ValueError, match="steady_states"):
            phoenix_amd.steady_states(net, bad)
    for kw in (dict(), dict(clamp=[0, -1, (1, 2)]), dict(tau0=float("inf"), max_iter=3, return_reduced=True)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.steady_states(net, y, **kw)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.reduced_jacobian(net, y)
    for kw in (dict(genes=[16]), dict(genes=[-1]), dict(genes=[]), dict(genes=[1], value=[1.0, 2.0]), dict(genes=[1], rows_per_call=0)):
        with pytest.raises(ValueError, match="knockout_steady_states"):
            phoenix_amd.knockout_steady_states(net, y, **kw)
    with pytest.raises(TypeError, match="knockout_steady_states"):
        phoenix_amd.knockout_steady_states(net, y, [1], clamp=[0, 1, 2])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.knockout_steady_states(net, y, [1, 2])
