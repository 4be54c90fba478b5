"""GPU tests of the implicit adjoint of the steady-state solve: each kernel of phx_steady_adj.hip
against its float64 formulas under a derived bound, phx_steady_param_grads against phx_rhs_vjp, the gradients of
`steady_states(differentiable=True)` against `steady_states_adjoint_reference` at the device's own steady states, the exact
zeros and the bits of a backward pass, and the default path.  Models and float64 formulas: tests/test_steady_cpu.py."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_net
from test_steady_cpu import make_model, moving, parts64, reference

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (N, H, B).  The last three are about the rows, which phx_steady_param_grads stages 32 at a time and cuts into segments of at
# least two chunks: 37 and 70 cross one and two chunk lengths (32, 64) inside one segment and are no multiples of 4 (the rows
# of an MFMA step); 131 rows are five chunks in two segments (two chunks and three).  The chunk length the kernel ended up
# with is 32, so the row counts the issue proposed straddle it as they are.
SHAPES = [(33, 1, 1), (37, 5, 3), (97, 7, 5), (96, 56, 4), (70, 97, 3), (200, 200, 2), (513, 97, 2), (130, 40, 37), (97, 7, 70),
          (37, 5, 131)]
FIELDS = ("Ws", "bs", "Wp", "bp", "Wa")


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def engine_params(net):
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    return engine.params_cached(*params_of(net))


_IN = {}


def kernel_inputs(N, H, B):
    """float32 inputs of the three kernels near a consistent adjoint state, and their float64 truth: the model and the steady
    states of `reference`, m = 1 on the moving genes (and a last row of weight 0 where B >= 2), Gaussian cotangents, q and
    hid of the float64 formulas rounded to float32.  Computed once per shape."""
    if (N, H, B) in _IN:
        return _IN[(N, H, B)]
    import phoenix_amd
    p, y0, held, ref = reference(N, H, B)
    y = ref.y.astype(np.float32)
    m = moving(p, held, B).astype(np.float32)
    if B >= 2:
        m[B - 1] = 0.0
    gy = np.random.default_rng(1000 + N).standard_normal((B, N)).astype(np.float32)
    adj = phoenix_amd.steady_states_adjoint_reference(p, y, gy, clamp=held)
    q = adj.q.astype(np.float32)
    hid = parts64(p, y)[4].astype(np.float32)
    _IN[(N, H, B)] = (p, y, m, gy, q, hid)
    return _IN[(N, H, B)]


def back64(p, y, m, gy, q, hid):
    """(u, A) float64: u = gy + C^T q on the float32 inputs and the same formula on absolute values"""
    H = p["Ws"].shape[0]
    w = {k: v.astype(np.float64) for k, v in p.items()}
    _, _, da, dl, _, _ = parts64(p, y)
    q, hid, gy = q.astype(np.float64), hid.astype(np.float64), gy.astype(np.float64)
    qv = q[:, H:] * hid[:, H:]
    u = gy + da * (q[:, :H] @ w["Ws"]) + dl * (qv @ w["Wp"])
    A = np.abs(gy) + da * (np.abs(q[:, :H]) @ np.abs(w["Ws"])) + dl * (np.abs(qv) @ np.abs(w["Wp"]))
    return u, A


def pgrads64(p, y, lam, q, hid):
    """({name: float64 product}, {name: the same on absolute values}) on the float32 inputs"""
    H = p["Ws"].shape[0]
    a, l = parts64(p, y)[:2]
    lam, q, hid = lam.astype(np.float64), q.astype(np.float64), hid.astype(np.float64)
    qv = q[:, H:] * hid[:, H:]

    def products(lam, qs, qv, hid, a, l):
        return {"Ws": qs.T @ a, "bs": qs.sum(axis=0), "Wp": qv.T @ l, "bp": qv.sum(axis=0), "Wa": lam.T @ hid}
    return products(lam, q[:, :H], qv, hid, a, l), products(np.abs(lam), np.abs(q[:, :H]), np.abs(qv), np.abs(hid), np.abs(a), np.abs(l))


# roundings of a term besides those of the sum, for y in [-1, 2] (correctly rounded + - * /, log1pf to 2 ulp):
#   project  the product m gy: 1, and one of slack                                                             -> 2
#   back     a', l' (y - 0.5, 1 + |s|, the products and the division, twice through d: 8), q v: 1, the fmas of the two
#            branches into gy and the product with m: 3                                                        -> 12
#   products a = s / d: 3, and the product's own: 1 -> 4;  l = log1pf(a): 3 at a condition number <= 1.7, 2 ulp of log1pf, q v
#            and the product's own: 2 -> 10 (taken for every product: the bias and Wa rows need 2)             -> 10
C_PROJECT, C_BACK, C_PRODUCTS = 2, 12, 10


def pgrads_bar(B, A):
    return {k: gamma(B + C_PRODUCTS) * v for k, v in A.items()}


@pytest.mark.parametrize("N,H,B", SHAPES)
def test_each_kernel_against_float64(pa, dev, N, H, B):
    """|got - ref64| <= gamma_k A with gamma_k = k u / (1 - k u), u = 2^-24, A the formula on absolute values, k the length of
    the contraction (any summation order) plus the roundings of a term counted above: N + 2 for the projection, 2H + 12 for
    lam and gy0, B + 10 for the parameter products.  Where A is 0 the result is exactly 0."""
    from phoenix_amd import engine
    p, y, m, gy, q, hid = kernel_inputs(N, H, B)
    P = engine_params(make_net(pa, dev, p))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    worst = {}

    def hold(name, got, ref, A, k):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape and np.all(np.isfinite(got)), name
        assert np.all(got[A == 0] == 0), name
        if (A > 0).any():
            worst[name] = float((np.abs(got - ref)[A > 0] / (gamma(k) * A[A > 0])).max())

    # the projection; a gene of weight 0 is not read: its cotangent may hold anything
    gy_nan = np.where(m == 0, np.float32(np.nan), gy)
    b = engine.steady_adjoint_project(P, t(m), t(gy_nan))
    mg = (m * gy).astype(np.float64)
    wa = p["Wa"].astype(np.float64)
    hold("b", b, mg @ wa, np.abs(mg) @ np.abs(wa), N + C_PROJECT)
    # lam and gy0
    lam, gy0 = engine.steady_adjoint_back(P, t(y), t(m), t(gy), t(q), t(hid))
    u, A = back64(p, y, m, gy, q, hid)
    hold("lam", lam, np.where(m != 0, u, 0), np.where(m != 0, A, 0), 2 * H + C_BACK)
    hold("gy0", gy0, np.where(m != 0, 0, u), np.where(m != 0, 0, A), 2 * H + C_BACK)
    assert not lam[t(m) == 0].any() and not gy0[t(m) != 0].any()
    # the parameter products, on float32 lam
    lam32 = lam.cpu().numpy()
    grads = engine.steady_param_grads(P, t(y), lam, t(q), t(hid))
    ref, A = pgrads64(p, y, lam32, q, hid)
    for k in FIELDS:
        hold(k, getattr(grads, k), ref[k], A[k], B + C_PRODUCTS)
    assert not grads.g.any() and grads.g.shape == (N,)
    print("(%d, %d, %d): worst error / bound %s" % (N, H, B, {n: "%.3f" % v for n, v in worst.items()}))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)


@pytest.mark.parametrize("N,H,B", [(37, 5, 3), (130, 40, 37), (37, 5, 131), (513, 97, 2)])
def test_bits_layouts_and_accumulation(pa, dev, N, H, B):
    from phoenix_amd import _lib, engine
    import ctypes as C
    p, y, m, gy, q, hid = (x if isinstance(x, dict) else torch.from_numpy(x).to(dev) for x in kernel_inputs(N, H, B))
    P = engine_params(make_net(pa, dev, p))
    b = engine.steady_adjoint_project(P, m, gy)
    lam, gy0 = engine.steady_adjoint_back(P, y, m, gy, q, hid)
    g1 = engine.steady_param_grads(P, y, lam, q, hid)
    # twice the same bits; a row's projection depends neither on B nor on its neighbours
    assert torch.equal(b, engine.steady_adjoint_project(P, m, gy))
    assert torch.equal(g1.flat, engine.steady_param_grads(P, y, lam, q, hid).flat)
    assert torch.equal(b[:1], engine.steady_adjoint_project(P, m[:1], gy[:1]))
    assert torch.equal(b.flip(0), engine.steady_adjoint_project(P, m.flip(0).contiguous(), gy.flip(0).contiguous()))
    assert torch.equal(lam[B - 1:], engine.steady_adjoint_back(P, y[B - 1:], m[B - 1:], gy[B - 1:], q[B - 1:], hid[B - 1:])[0])
    # a row with lam = 0 and q = 0 contributes exact zeros: the batch with such a row appended (the segments stay as they are)
    size = _lib.load().phx_steady_param_grads_workspace_bytes
    assert size(N, H, B) == size(N, H, B + 1)
    y2, l2, q2, h2 = (torch.cat([x, torch.zeros_like(x[:1])]) for x in (y, lam, q, hid))
    y2[B:] = 0.25
    h2[B:] = 3.0
    assert torch.equal(g1.flat, engine.steady_param_grads(P, y2, l2, q2, h2).flat)
    # accumulation: a second call adds to the first one's buffers
    g2 = engine.steady_param_grads(P, y, lam, q, hid)
    engine.steady_param_grads(P, y, lam, q, hid, grads=g2)
    assert torch.equal(g2.flat, g1.flat + g1.flat)
    # the WaT layout of phx_grads
    g3 = P.new_grads()
    waT = torch.empty((2 * H, N), dtype=torch.float32, device=dev)
    g3.c.WaT, g3.c.Wa = waT.data_ptr(), None
    nbytes = _lib.load().phx_steady_param_grads_workspace_bytes(N, H, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = _lib.load().phx_steady_param_grads(C.byref(P.c), y.data_ptr(), lam.data_ptr(), q.data_ptr(), hid.data_ptr(), B,
                                            C.byref(g3.c), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(waT.t(), g1.Wa) and torch.equal(g3.Ws, g1.Ws) and torch.equal(g3.bp, g1.bp)


@pytest.mark.parametrize("N,H,B", [(37, 5, 3), (97, 7, 5), (96, 56, 4), (70, 97, 3), (130, 40, 37)])
def test_param_grads_against_rhs_vjp(pa, dev, N, H, B):
    """phx_rhs_vjp with cot = lam / relu(g) on the moving genes forms the same five products from z = WaT (g cot) and its own
    hidden vector: an independent kernel family.  The two agree within the sum of their derived bounds:
      ours    gamma_(B + 11) A (test_each_kernel_against_float64, and the rounding of q = fl(z64) to float32);
      theirs  z_j carries gamma_(N + 4) (|Wa|^T |lam|)_j (an N-term contraction, cot = lam / g and g cot: 2 roundings), the sums
              half of hid gamma_(N + 8) (|Ws| |a| + |bs|), v_j the relative error rel_j = expm1(gamma_(N + 18) (|Wp| |l| + |bp|))
              + 4 u of tests/test_steady_gpu.py, a and l the roundings counted above, and the sum over the rows gamma_(B + 12).
    The g output of phx_rhs_vjp is ignored."""
    from phoenix_amd import engine
    p, y, m, gy, q, hid = kernel_inputs(N, H, B)
    w = {k: v.astype(np.float64) for k, v in p.items()}
    P = engine_params(make_net(pa, dev, p))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    lam = engine.steady_adjoint_back(P, t(y), t(m), t(gy), t(q), t(hid))[0].cpu().numpy()
    gpos = np.maximum(p["g"], 0)
    cot = np.where(m != 0, lam / np.where(gpos > 0, gpos, 1), 0).astype(np.float32)
    lam = (cot.astype(np.float64) * gpos).astype(np.float32)          # what phx_rhs_vjp contracts, to one rounding
    z64 = lam.astype(np.float64) @ w["Wa"]                            # the consistent q = Wa^T lam
    hid64 = parts64(p, y)[4]
    ours = engine.steady_param_grads(P, t(y), t(lam), t(z64.astype(np.float32)), t(hid64.astype(np.float32)))
    _, theirs = engine.rhs_vjp(P, t(y), t(cot))
    ref, A = pgrads64(p, y, lam, z64, hid64)
    a, l = np.abs(parts64(p, y)[0]), np.abs(parts64(p, y)[1])
    rel_v = np.expm1(gamma(N + 18) * (l @ np.abs(w["Wp"]).T + np.abs(w["bp"]))) + 4 * U
    dhid = np.concatenate([gamma(N + 8) * (a @ np.abs(w["Ws"]).T + np.abs(w["bs"])), hid64[:, H:] * rel_v], axis=1)
    dz = gamma(N + 4) * (np.abs(lam.astype(np.float64)) @ np.abs(w["Wa"]))
    v = hid64[:, H:]
    dzv = dz[:, H:] * v * (1 + rel_v) + np.abs(z64[:, H:]) * v * rel_v
    one = np.ones((B, 1))
    theirs_bar = {"Wa": np.abs(lam).T.astype(np.float64) @ dhid, "Ws": dz[:, :H].T @ a, "bs": (dz[:, :H].T @ one)[:, 0],
                  "Wp": dzv.T @ l, "bp": (dzv.T @ one)[:, 0]}
    worst = {}
    for k in FIELDS:
        bar = gamma(B + C_PRODUCTS + 1) * A[k] + theirs_bar[k] + gamma(B + 12) * A[k]
        got, other = getattr(ours, k).cpu().numpy().astype(np.float64), getattr(theirs, k).cpu().numpy().astype(np.float64)
        assert got.shape == other.shape == ref[k].shape
        ok = bar > 0
        assert np.all(got[~ok] == other[~ok])
        worst[k] = (float((np.abs(got - other)[ok] / bar[ok]).max()), float(np.abs(got - ref[k]).max()), float(np.abs(other - ref[k]).max()))
    print("(%d, %d, %d): |ours - rhs_vjp| / bound, |ours - ref64|, |rhs_vjp - ref64|: %s"
          % (N, H, B, {k: "%.3f %.1e %.1e" % v for k, v in worst.items()}))
    for k, v in worst.items():
        assert v[0] <= 1.0, (k, v)


# --------------------------------------------------------------------------- end to end
def run(pa, dev, N, H, B, G=None, **kw):
    """steady_states(differentiable=True) on the test model and (y* G).sum().backward() -> (net, y0 tensor, result, G)"""
    p, y0, held = make_model(N, H, B)
    net = make_net(pa, dev, p)
    for q in net.parameters():
        q.requires_grad_(True)
        q.grad = None
    y0t = torch.from_numpy(y0).to(dev).requires_grad_(True)
    out = pa.steady_states(net, y0t, clamp=held, differentiable=True, **kw)
    if G is None:
        G = np.random.default_rng(1000 + N).standard_normal((B, N)).astype(np.float32)
    (out.y * torch.from_numpy(G).to(dev)).sum().backward()
    return p, held, net, y0t, out, G


def device_grads(net, y0t):
    from phoenix_amd.odenet import params_of
    ws, bs, wp, bp, wa, g = params_of(net)
    f = lambda x: None if x.grad is None else x.grad.detach().cpu().numpy()      # noqa: E731
    return {"y0": f(y0t), "Ws": f(ws), "bs": f(bs), "Wp": f(wp), "bp": f(bp), "Wa": f(wa), "g": f(g)}


@pytest.mark.parametrize("N,H,B", SHAPES[:9])
def test_gradients_against_the_reference_at_the_devices_own_steady_states(pa, dev, N, H, B):
    """Every gradient against steady_states_adjoint_reference in float64 at the device's y* (the conditioning of the forward
    problem does not enter).  Scale: the distance of the float32 reference from the float64 one at the same y* and gy -- the
    arithmetic's own error.  The device stays within 8 x that distance plus gamma_B times the absolute sums (three float32
    contractions are chained and the solve is in double: 8 is headroom, not a fit)."""
    p, held, net, y0t, out, G = run(pa, dev, N, H, B)
    assert out.y.requires_grad and not out.residual.requires_grad and not out.status.requires_grad
    assert bool((out.status == 0).all()) and bool((pa.last_backward_info() == 0).all())
    ystar = out.y.detach().cpu().numpy()
    r64 = pa.steady_states_adjoint_reference(p, ystar, G, clamp=held)
    r32 = pa.steady_states_adjoint_reference(p, ystar, G, clamp=held, dtype=np.float32)
    got = device_grads(net, y0t)
    _, A = pgrads64(p, ystar, r64.lam, r64.q, parts64(p, ystar)[4])
    A["y0"] = back64(p, ystar, None, G, r64.q, parts64(p, ystar)[4])[1]
    report = {}
    for k in ("y0",) + FIELDS:
        ref = getattr(r64, k)
        assert got[k].shape == ref.shape or k == "g", k
        d32 = float(np.abs(getattr(r32, k).astype(np.float64) - ref).max())
        ddev = float(np.abs(got[k].astype(np.float64) - ref).max())
        report[k] = (ddev, d32, 8 * d32 + gamma(B) * float(A[k].max()))
    print("(%d, %d, %d): |device - ref64|, |ref32 - ref64|, bound: %s"
          % (N, H, B, {k: "%.2e %.2e %.2e" % v for k, v in report.items()}))
    for k, v in report.items():
        assert v[0] <= v[2], (k, v)
    assert got["g"] is None or not got["g"].any()


def test_structure_on_the_device(pa, dev):
    N, H, B = 97, 7, 5
    p, held, net, y0t, out, G = run(pa, dev, N, H, B)
    first = device_grads(net, y0t)
    free = moving(p, held, B)
    assert first["g"] is None or not first["g"].any()
    assert not first["y0"][free].any() and first["y0"][~free].all()
    p, held, net2, y0t2, out2, _ = run(pa, dev, N, H, B)
    second = device_grads(net2, y0t2)
    for k, v in first.items():
        assert (v is None and second[k] is None) or np.array_equal(v, second[k]), k
    # [B, 1, N] states get a [B, 1, N] gradient
    net3 = make_net(pa, dev, p)
    y3 = y0t.detach().reshape(B, 1, N).clone().requires_grad_(True)
    pa.steady_states(net3, y3, clamp=held, differentiable=True).y.sum().backward()
    assert y3.grad.shape == (B, 1, N)


def test_rows_that_did_not_converge_contribute_nothing(pa, dev):
    N, H, B = 97, 7, 5
    kw = dict(max_iter=1)
    p, held, net, y0t, out, G = run(pa, dev, N, H, B, **kw)
    status = out.status.cpu().numpy()
    if (status == 0).all() or (status != 0).all():      # one step from y0 under a tolerance some rows meet and some do not
        rho = np.sort(out.residual.cpu().numpy())
        kw = dict(max_iter=1, tol=float((rho[0] + rho[-1]) / 2))
        p, held, net, y0t, out, G = run(pa, dev, N, H, B, **kw)
        status = out.status.cpu().numpy()
    assert (status == 0).any() and (status != 0).any(), status
    info = pa.last_backward_info()
    assert info.dtype == torch.int32 and info.is_cuda and info.shape == (B,)
    assert np.array_equal(info.cpu().numpy(), np.where(status == 0, 0, -2))
    first = device_grads(net, y0t)
    assert not first["y0"][status != 0].any() and first["y0"][status == 0].any()
    G0 = np.where(status[:, None] == 0, G, np.float32(0))
    _, _, net2, y0t2, out2, _ = run(pa, dev, N, H, B, G=G0, **kw)
    assert torch.equal(out.y, out2.y)
    second = device_grads(net2, y0t2)
    for k in FIELDS + ("y0",):
        assert np.array_equal(first[k], second[k]), k
    assert np.abs(first["Wa"]).max() > 0


@pytest.mark.parametrize("N,H,B", [(37, 5, 3), (70, 97, 3)])
def test_the_default_path_is_unchanged(pa, dev, N, H, B):
    p, y0, held = make_model(N, H, B)
    net = make_net(pa, dev, p)
    y0t = torch.from_numpy(y0).to(dev)
    for kw in (dict(), dict(max_iter=0), dict(max_iter=3, return_reduced=True)):
        plain = pa.steady_states(net, y0t, clamp=held, **kw)
        diff = pa.steady_states(net, y0t, clamp=held, differentiable=True, **kw)
        for a, b in zip(plain, diff):
            assert (a is None and b is None) or (torch.equal(a.detach(), b.detach()) and not a.requires_grad), kw
        assert diff.y.requires_grad and not any(x.requires_grad for x in diff[1:5])
        assert plain.y.data_ptr() != y0t.data_ptr()
