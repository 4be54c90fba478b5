"""GPU tests of the standalone RHS evaluation, its VJP and the fused prior loss against the float64 truth of
tests/test_rhs_truth_cpu.py, entry by entry under the bars derived there: phx_rhs_forward, phx_rhs_vjp, phx_prior_mse,
phx_prior_mse_save and phx_prior_vjp_saved on every route the library has for them -- the kernel chain of
phx_mfma_batch.inc (k2_hidden_partials -> k2_hidden_reduce -> k2_expand / k2_expand_vjp / k2_pgrad_contract, with and
without the packed weight images), the pass-structured k1_eval_fwd / k1_eval_pgrad, and the VALU k_eval -- at the launch
edges `test_every_shape_has_its_edge` names, on inputs whose entries span three decades.  Every test prints the worst
|error| / bar of each output before it asserts that none exceeds 1; an entry whose bar is 0 must be exactly 0.

Measured on an MI355X: worst |error| / bar over each group's cases (60 cases, 6 s; the two-chunk case 1.6 s each mode, of
which the float64 truth is 1.2 s):
    route                                  f      vjp_y  dWs    dbs    dWp    dbp    dWa    dg
    chain with images (test_default_route) 0.089  0.228  0.216  0.096  0.071  0.034  0.100  0.058
    chain, two row chunks, rows < 560      0.002  0.013  (gradients of the whole batch: all < 0.001)
    chain, two row chunks, rows >= 560     0.002  0.014
    k1_eval_fwd, k1_eval_pgrad (PHX_PGRAD) 0.089  -      0.023  0.011  0.021  0.011  0.085  0
    k1_eval_fwd beside the chain's VJP     0.089  0.228  0.025  0.015  0.027  0.014  0.085  0.023
    k_eval, VALU (libm bars)               0.089  0.118  0.025  0.019  0.020  0.014  0.051  0.024
    chain without weight images            0.067  0.228  0.012  0.006  0.016  0.007  0.035  0.023
    a row alone                            0.042  0.121
    fused loss: loss 0.002, cot 0.241; gradients from the saved sections and recomputed 0.004 at most, dg 0
The loss and cotangent with and without keep_hidden were bit-identical at all four shapes, and a row alone returned the
bits of its row of the full batch in all eight cases.  No entry was outside its bar and no exact zero was missed.
With one wrong line in a scratch build, run on the MI355X: the tail gene dropped in k2_hidden_partials fails 44 of the 60
cases (every case of test_default_route, test_second_row_chunk, test_fused_prior_loss, test_a_row_alone, and the
min_rows / no_wimg cases of test_other_routes); hb = 0 in the second hidden chunk of launch_batch_vjp fails the ten cases
with H > 128 (test_default_route at H = 129, 224, 225, 256 and test_a_row_alone at H = 129); first_chunk = 1 on every row
chunk fails test_second_row_chunk[False]."""
import time

import numpy as np
import pytest
import torch

from test_gpu_parity import make_net
from test_rhs_truth_cpu import (PRIOR_SHAPES, ROUTE_SHAPES, ROW_SHAPES, SHAPES, TWO_CHUNK_SHAPE, loss_truth, make_inputs,
                                make_target, plan_batch, truth, worst_ratio)

pytestmark = pytest.mark.gpu
GRADS = ("Ws", "bs", "Wp", "bp", "Wa", "g")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


_TRUTH = {}


def truth_of(N, H, B, prior_only, kind="fast"):
    """the truth of a shape's inputs, computed once per session and never written to"""
    key = (N, H, B, prior_only, kind)
    if key not in _TRUTH:
        _TRUTH[key] = truth(*make_inputs(N, H, B), prior_only, kind=kind)
    return _TRUTH[key]


def device_inputs(pa, dev, N, H, B):
    from phoenix_amd import engine
    p, y, cot = make_inputs(N, H, B)
    P = engine.params_cached(*pa.odenet.params_of(make_net(pa, dev, p)))
    return p, P, torch.from_numpy(y).to(dev), torch.from_numpy(cot).to(dev)


def evaluate(P, y, cot, prior_only, forward=True, calls=("all", "vjp", "grads")):
    """[(label, output, tensor)] of the entry points: rhs_forward, and rhs_vjp with everything asked for (f_out included), with
    the input VJP alone, with the gradients alone (in prior_only that call is the gradient chain without kernel E)"""
    from phoenix_amd import engine
    out = []
    if forward:
        out.append(("rhs_forward", "f", engine.rhs_forward(P, y, prior_only)))
    if "all" in calls:
        fo = torch.empty_like(y)
        v, g = engine.rhs_vjp(P, y, cot, prior_only, f_out=fo)
        out += [("f_out", "f", fo), ("vjp_y", "vjp_y", v)] + [("d" + k, k, getattr(g, k)) for k in GRADS]
    if "vjp" in calls:
        v, none = engine.rhs_vjp(P, y, cot, prior_only, want_grads=False)
        assert none is None
        out.append(("vjp_y alone", "vjp_y", v))
    if "grads" in calls:
        none, g = engine.rhs_vjp(P, y, cot, prior_only, want_vjp_y=False)
        assert none is None
        out += [("d%s alone" % k, k, getattr(g, k)) for k in GRADS]
    torch.cuda.synchronize()
    return out


def hold(tag, results, t, rows=None):
    """prints worst |error| / bar per output and asserts <= 1; rows: also per side of a row boundary, for f and vjp_y"""
    worst = {}
    for label, k, got in results:
        got = got.detach().cpu().numpy()
        ref, bar = t[k]
        worst[label] = worst_ratio(got, ref, bar)
        if rows is not None and k in ("f", "vjp_y"):
            got = got.reshape(ref.shape)
            worst[label] = "%.3f below row %d, %.3f from it" % (worst_ratio(got[:rows], ref[:rows], bar[:rows]), rows,
                                                                worst_ratio(got[rows:], ref[rows:], bar[rows:]))
    print("%s: worst |error| / bar %s" % (tag, {k: v if isinstance(v, str) else "%.3f" % v for k, v in worst.items()}))
    for label, k, got in results:
        assert worst_ratio(got.detach().cpu().numpy(), *t[k]) <= 1.0, (tag, label)
    return worst


def hold_zeros(p, results, cot, prior_only):
    """the exact zeros by name (the bars say the same: they are 0 there)"""
    gz = torch.from_numpy(p["g"] <= 0)
    B, N = cot.shape
    for label, k, got in results:
        got = got.detach().cpu()
        if k == "g" and prior_only:
            assert not got.any(), label
        if not prior_only and k == "f":
            assert not got.reshape(B, N)[:, gz].any(), label
        if not prior_only and k == "g":
            assert not got[gz].any(), label
        if k == "vjp_y" and B >= 3:
            assert not got.reshape(B, N)[B // 2].any(), label        # the zero cotangent row
        if k == "Wa":
            assert not got[N // 2].any(), label                      # the zero cotangent column


@pytest.mark.parametrize("prior_only", [False, True])
@pytest.mark.parametrize("N,H,B,edge", SHAPES)
def test_default_route(pa, dev, N, H, B, edge, prior_only):
    """the kernel chain A -> R -> D / E / C with the packed weight images, which every batch size takes by default"""
    p, P, y, cot = device_inputs(pa, dev, N, H, B)
    res = evaluate(P, y, cot, prior_only)
    hold("(%d, %d, %d) %s, prior_only=%s" % (N, H, B, edge, prior_only), res, truth_of(N, H, B, prior_only))
    hold_zeros(p, res, cot, prior_only)


@pytest.mark.parametrize("prior_only", [False, True])
def test_second_row_chunk(pa, dev, prior_only):
    """launch_batch_forward and launch_batch_vjp with t0 > 0: the smallest shape in which both take two row chunks"""
    N, H, B = TWO_CHUNK_SHAPE
    pl = plan_batch(N, H, B)
    assert pl["chunk_tiles"] < pl["ntiles"] and pl["chunk_tiles2"] < pl["ntiles"] and pl["chunk_tiles"] == pl["chunk_tiles2"]
    t0 = time.time()
    p, P, y, cot = device_inputs(pa, dev, N, H, B)
    t = truth(*make_inputs(N, H, B), prior_only)             # (not kept: a gigabyte with its bars)
    t1 = time.time()
    res = evaluate(P, y, cot, prior_only, calls=("all",))
    t2 = time.time()
    hold("(%d, %d, %d) two row chunks of %d tiles, prior_only=%s" % (N, H, B, pl["chunk_tiles"], prior_only), res, t,
         rows=16 * pl["chunk_tiles"])
    hold_zeros(p, res, cot, prior_only)
    print("inputs and float64 truth %.1f s, device calls %.1f s, comparison %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))


@pytest.mark.parametrize("N,H,B", PRIOR_SHAPES)
def test_fused_prior_loss(pa, dev, N, H, B):
    """prior_mse with and without the saved hidden sections, then the backward from them (H <= 128) and the one that
    recomputes them: the loss, the cotangent, and the five gradients of sum(cot * prior_only_forward(X)) for the cotangent
    the device returned; dg is exactly 0"""
    from phoenix_amd import engine
    p, P, X, _ = device_inputs(pa, dev, N, H, B)
    tgt = make_target(N, H, B)
    T = torch.from_numpy(tgt).to(dev)
    loss0, cot0 = engine.prior_mse(P, X, T)
    loss1, cot1, z = engine.prior_mse(P, X, T, keep_hidden=True)
    assert (z is None) == (H > 128)
    loss64, bar_loss, cot64, bar_cot = loss_truth(p, X.cpu().numpy(), tgt)
    same = torch.equal(loss0, loss1) and torch.equal(cot0, cot1)
    wl = {n: abs(float(v) - loss64) / bar_loss for n, v in (("loss", loss0), ("loss, keep_hidden", loss1))}
    wl.update({n: worst_ratio(v.cpu().numpy(), cot64, bar_cot) for n, v in (("cot", cot0), ("cot, keep_hidden", cot1))})
    print("(%d, %d, %d) fused loss: worst |error| / bar %s; with and without keep_hidden bit-identical: %s"
          % (N, H, B, {k: "%.3f" % v for k, v in wl.items()}, same))
    assert max(wl.values()) <= 1.0, wl
    t = truth(p, X.cpu().numpy(), cot1.cpu().numpy(), True)
    res = []
    if z is not None:
        g = engine.prior_vjp_saved(P, X, cot1, z)
        res += [("d%s saved" % k, k, getattr(g, k)) for k in GRADS]
    g = engine.rhs_vjp(P, X, cot0, True, want_grads=True, want_vjp_y=False)[1]
    res += [("d%s recomputed" % k, k, getattr(g, k)) for k in GRADS]
    torch.cuda.synchronize()
    hold("(%d, %d, %d) gradients of the loss" % (N, H, B), res, t)
    for label, k, got in res:
        assert k != "g" or not got.any(), label


ROUTES = [(r,) + s for r in ("pgrad_v1", "min_rows", "v0") for s in ROUTE_SHAPES] + [("no_wimg",) + s for s in (ROUTE_SHAPES[1], ROUTE_SHAPES[2])]


@pytest.mark.parametrize("prior_only", [False, True])
@pytest.mark.parametrize("route,N,H,B", ROUTES)
def test_other_routes(pa, dev, monkeypatch, route, N, H, B, prior_only):
    """the same truth and bars on the routes the library's switches select:
    pgrad_v1: PHX_PGRAD=v1, k1_eval_fwd for the forward and k1_eval_pgrad for the gradients of prior_only_forward (every
              PHX_EVAL_NBC at H <= 48); min_rows: PHX_BATCH_MIN_ROWS above the batch, k1_eval_fwd beside the chain's VJP;
    v0: PHX_ENGINE=v0, the VALU k_eval with libm activations (the libm constants); no_wimg: the chain staging its weights
    from the parameter arrays, as a C caller without packed images gets it (PHX_BATCH_MIN_ROWS=1 keeps the forward on it)"""
    p, P, y, cot = device_inputs(pa, dev, N, H, B)
    tag = "(%d, %d, %d) %s, prior_only=%s" % (N, H, B, route, prior_only)
    if route == "pgrad_v1":
        monkeypatch.setenv("PHX_PGRAD", "v1")
        res = evaluate(P, y, cot, prior_only, calls=())
        if prior_only:
            for nbc in ((2, 3, 4) if H <= 48 else (None,)):
                if nbc is not None:
                    monkeypatch.setenv("PHX_EVAL_NBC", str(nbc))
                res += [("%s, NBC %s" % (a, nbc), b, c) for a, b, c in evaluate(P, y, cot, True, forward=False, calls=("grads",))]
        t = truth_of(N, H, B, prior_only)
    elif route == "min_rows":
        monkeypatch.setenv("PHX_BATCH_MIN_ROWS", "100000")
        res, t = evaluate(P, y, cot, prior_only, calls=("all",)), truth_of(N, H, B, prior_only)
    elif route == "v0":
        monkeypatch.setenv("PHX_ENGINE", "v0")
        res, t = evaluate(P, y, cot, prior_only, calls=("all",)), truth_of(N, H, B, prior_only, "libm")
    else:
        monkeypatch.setenv("PHX_BATCH_NO_WIMG", "1")
        monkeypatch.setenv("PHX_BATCH_MIN_ROWS", "1")
        res, t = evaluate(P, y, cot, prior_only), truth_of(N, H, B, prior_only)
    hold(tag, res, t)
    hold_zeros(p, res, cot, prior_only)


@pytest.mark.parametrize("prior_only", [False, True])
@pytest.mark.parametrize("N,H,B", ROW_SHAPES)
def test_a_row_alone(pa, dev, N, H, B, prior_only):
    """rows 0 and B - 1 as batches of one row: f and vjp_y within the bars of those rows; whether they are also the bits
    of the same rows of the full batch is printed, not asserted (the code does not promise it)"""
    from phoenix_amd import engine
    p, P, y, cot = device_inputs(pa, dev, N, H, B)
    t = truth_of(N, H, B, prior_only)
    full_f = engine.rhs_forward(P, y, prior_only)
    full_v = engine.rhs_vjp(P, y, cot, prior_only, want_grads=False)[0]
    for b in (0, B - 1):
        f1 = engine.rhs_forward(P, y[b:b + 1].contiguous(), prior_only)
        fo = torch.empty_like(f1)
        v1 = engine.rhs_vjp(P, y[b:b + 1].contiguous(), cot[b:b + 1].contiguous(), prior_only, want_grads=False, f_out=fo)[0]
        torch.cuda.synchronize()
        tb = {k: (t[k][0][b:b + 1], t[k][1][b:b + 1]) for k in ("f", "vjp_y")}
        hold("(%d, %d, %d) row %d alone, prior_only=%s" % (N, H, B, b, prior_only),
             [("rhs_forward", "f", f1), ("f_out", "f", fo), ("vjp_y", "vjp_y", v1)], tb)
        print("    bit-identical to the row of the full batch: f %s, vjp_y %s"
              % (torch.equal(f1, full_f[b:b + 1]), torch.equal(v1, full_v[b:b + 1])))
