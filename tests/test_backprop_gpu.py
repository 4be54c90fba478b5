"""Backward pass of `odeint(method="euler" | "midpoint" | "rk4")`: backpropagation through the fixed-grid steps (the
discrete adjoint, k1_solve_bp) against G18 (tests/golden/make_golden_backprop.py: the reference's own `odeint`
differentiated by `.backward()`), on the MI355X.  Run with `-m gpu`.  Everything goes through the public `odeint`."""

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub

pytestmark = pytest.mark.gpu

KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")
TOL_FIXED = 1e-5      # the project's fixed-grid bar (tests/test_substeps_gpu.py)
HS = (0.5, 0.75, 0.125, 0.3, None)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


@pytest.fixture(scope="module")
def g18():
    return load_golden("g18_backprop")


def make_net(pa, dev, p):
    H, N = p["Ws"].shape
    net = pa.ODENet(dev, N, neurons=H)
    with torch.no_grad():
        net.net_sums.linear_out.weight.copy_(torch.from_numpy(p["Ws"]))
        net.net_sums.linear_out.bias.copy_(torch.from_numpy(p["bs"]))
        net.net_prods.linear_out.weight.copy_(torch.from_numpy(p["Wp"]))
        net.net_prods.linear_out.bias.copy_(torch.from_numpy(p["bp"]))
        net.net_alpha_combine.linear_out.weight.copy_(torch.from_numpy(p["Wa"]))
        net.gene_multipliers.copy_(torch.from_numpy(p["g"]).reshape(1, N))
    return net


def grads_of(net):
    def g(p):
        return (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().numpy()
    return {"Ws": g(net.net_sums.linear_out.weight), "bs": g(net.net_sums.linear_out.bias),
            "Wp": g(net.net_prods.linear_out.weight), "bp": g(net.net_prods.linear_out.bias),
            "Wa": g(net.net_alpha_combine.linear_out.weight), "g": g(net.gene_multipliers).reshape(-1)}


def zero_grads(net):
    for p in net.parameters():
        p.grad = None


def rand_params(N, H, seed, std=0.1, neg=0.1):
    r = np.random.RandomState(seed)
    g = r.rand(N).astype(np.float32)
    g[r.rand(N) < neg] *= -1
    return {"Ws": (r.randn(H, N) * std).astype(np.float32), "bs": r.uniform(-.2, .2, H).astype(np.float32),
            "Wp": (r.randn(H, N) * std).astype(np.float32), "bp": r.uniform(-.2, .2, H).astype(np.float32),
            "Wa": (r.randn(N, 2 * H) * std).astype(np.float32), "g": g}


def opts(h):
    return None if h is None else {"step_size": h}


def run_odeint(pa, net, y0, t, G, method, h, fn=None):
    """solution and the seven gradients of sum(G * odeint(...)) through the public entry point"""
    zero_grads(net)
    y0r = y0.clone().requires_grad_(True)
    sol = (fn or pa.odeint)(net, y0r, t, method=method, options=opts(h))
    (sol * G).sum().backward()
    out = {"sol": sol.detach().cpu().numpy(), "grad_y0": y0r.grad.cpu().numpy()}
    out.update({"grad_" + k: v for k, v in grads_of(net).items()})
    return out


def errors(got, want):
    return {k: relerr(got[k], want[k]) for k in ["sol", "grad_y0"] + ["grad_" + k for k in KEYS]}


# ------------------------------------------------------------------------------------------ 1: every golden case
@pytest.mark.parametrize("yname", ["single", "batch"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("tname", ["t2", "t5", "t_dec"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_g18_every_case(pa, dev, g18, method, tname, h, yname):
    net = make_net(pa, dev, sub(g18, "p_"))
    tag = "%s/%s/%s/%s" % (method, tname, "none" if h is None else repr(h), yname)
    c = sub(g18, tag + "/")
    y0 = torch.from_numpy(g18["y0_" + yname]).to(dev)
    t = torch.from_numpy(g18[tname]).to(dev)
    G = torch.from_numpy(g18["G/%s/%s" % (tname, yname)]).to(dev)
    errs = errors(run_odeint(pa, net, y0, t, G, method, h), c)
    spread = float(c["spread"])
    bar = max(TOL_FIXED, 2 * spread)      # the reference's own float32 rounding is the floor
    print(tag, "spread=%.2e bar=%.2e" % (spread, bar), " ".join("%s=%.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < bar, (tag, k, e, bar)


@pytest.mark.parametrize("name, h", [("h", 0.25), ("none", None)])
def test_g18_per_sample_grids(pa, dev, g18, name, h):
    """t [B, 2]: the reference's loop over samples (train_insilico.py:128-130) as one call"""
    net = make_net(pa, dev, sub(g18, "p_"))
    c = sub(g18, "ps/%s/" % name)
    y0 = torch.from_numpy(g18["y0_batch"]).to(dev)
    t = torch.from_numpy(g18["ps/t"]).to(dev)
    G = torch.from_numpy(g18["ps/G"]).to(dev).clone()
    G[0] = 0                                # the reference's loss reads the end state only
    got = run_odeint(pa, net, y0, t, G, "rk4", h)
    got["sol"] = got["sol"][1]
    errs = errors(got, c)
    bar = max(TOL_FIXED, 2 * float(c["spread"]))
    print("ps/" + name, "spread=%.2e" % float(c["spread"]), " ".join("%s=%.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < bar, (k, e, bar)


# ------------------------------------------------------------------------------------------ 2: discrete is not continuous
def test_discrete_gradient_is_not_the_continuous_adjoint(pa, dev, g18):
    """rk4, one step per interval: odeint(...).backward() and odeint_adjoint(...).backward() differ by more than ten times
    the bar, and each matches its own golden (G18; the adjoint's is G3, the same problem)"""
    net = make_net(pa, dev, sub(g18, "p_"))
    y0 = torch.from_numpy(g18["y0_batch"]).to(dev)
    t = torch.from_numpy(g18["t5"]).to(dev)
    G = torch.from_numpy(g18["G/t5/batch"]).to(dev)
    disc = run_odeint(pa, net, y0, t, G, "rk4", None)
    cont = run_odeint(pa, net, y0, t, G, "rk4", None, fn=pa.odeint_adjoint)
    c = sub(g18, "rk4/t5/none/batch/")
    bar = max(TOL_FIXED, 2 * float(c["spread"]))
    for k, e in errors(disc, c).items():
        assert e < bar, (k, e)
    assert np.array_equal(disc["sol"], cont["sol"])
    diffs = {k: relerr(cont[k], disc[k]) for k in disc if k != "sol"}
    print("continuous vs discrete:", " ".join("%s=%.2e" % kv for kv in diffs.items()))
    assert all(d > 10 * bar for d in diffs.values()), diffs
    # the continuous adjoint against ITS golden: the reference's odeint_adjoint on the same problem (G3, its own cotangent)
    g3 = load_golden("g3_fixed")
    assert np.array_equal(g3["p_Ws"], g18["p_Ws"]) and np.array_equal(g3["y0_batch"], g18["y0_batch"])
    c3 = sub(g3, "rk4/t5/batch/")
    cont3 = run_odeint(pa, net, y0, t, torch.from_numpy(c3["G"]).to(dev), "rk4", None, fn=pa.odeint_adjoint)
    for k, e in errors(cont3, c3).items():
        assert e < TOL_FIXED, (k, e)


# ------------------------------------------------------------------------------------------ 3, 4: full size, torch arbiter
class TorchNet(torch.nn.Module):
    """plain-torch restatement of ODENet.forward (odenet.py:85-91) in the dtype of its tensors"""

    def __init__(self, p, dev, dtype):
        super().__init__()
        for k in KEYS:
            setattr(self, k, torch.nn.Parameter(torch.from_numpy(p[k]).to(dev, dtype)))

    def forward(self, t, y):
        s = y - 0.5
        a = s / (1 + s.abs())
        sums = a @ self.Ws.t() + self.bs
        prods = torch.exp(torch.log1p(a) @ self.Wp.t() + self.bp)
        joint = torch.cat((sums, prods), dim=-1) @ self.Wa.t()
        return torch.relu(self.g) * (joint - y)


def arbiter(pa, p, dev, dtype, y0, t, G, method, h):
    """phoenix_amd.generic.integrate over TorchNet on the device, differentiated by autograd"""
    from phoenix_amd import generic
    net = TorchNet(p, dev, dtype)
    y0r = torch.from_numpy(y0).to(dev, dtype).requires_grad_(True)
    sol = generic.integrate(net, y0r, torch.from_numpy(t).to(dev), 1e-7, 1e-9, method, step_size=h)
    (sol * torch.from_numpy(G).to(dev, dtype)).sum().backward()
    out = {"sol": sol.detach().cpu().numpy(), "grad_y0": y0r.grad.cpu().numpy()}
    out.update({"grad_" + k: getattr(net, k).grad.cpu().numpy() for k in KEYS})
    return out


def check_against_arbiter(pa, dev, N, H, B, seed, h, tag):
    p = rand_params(N, H, seed=seed, std=0.05)
    net = make_net(pa, dev, p)
    r = np.random.RandomState(seed + 1)
    y0 = np.clip(r.beta(2, 2, size=(B, N)) + r.uniform(-0.25, 0.25, size=(1, N)), 0, 1).astype(np.float32)
    t = np.array([0.0, 2.0, 3.0, 7.0, 9.0], np.float32)
    G = (r.randn(5, B, N) / (B * N)).astype(np.float32)
    ref64 = arbiter(pa, p, dev, torch.float64, y0, t, G, "rk4", h)
    ref32 = arbiter(pa, p, dev, torch.float32, y0, t, G, "rk4", h)
    e32 = errors(ref32, ref64)
    got = run_odeint(pa, net, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(G).to(dev), "rk4", h)
    errs = errors(got, ref64)
    for k in errs:
        print("%s %-8s err=%.2e e32=%.2e" % (tag, k, errs[k], e32[k]))
    for k in errs:
        assert errs[k] < max(TOL_FIXED, 2 * e32[k]), (tag, k, errs[k], e32[k])


@pytest.mark.parametrize("h", [None, 0.75])
def test_full_size_insilico_vs_torch(pa, dev, h):
    """BASELINE configuration 2 (N=350, H=40, 1024 trajectories x 4 intervals, rk4): one step per interval, and a step size
    that gives interpolated outputs"""
    check_against_arbiter(pa, dev, 350, 40, 1024, 2, h, "C2/h=%s" % h)


@pytest.mark.parametrize("h", [None, 0.75])
def test_wide_hidden_ragged_batch_vs_torch(pa, dev, h):
    """48 < H <= 128 (the eight-tile kernel) and a batch that is no multiple of 16"""
    check_against_arbiter(pa, dev, 200, 100, 37, 5, h, "H100/h=%s" % h)


# ------------------------------------------------------------------------------------------ 5: batch splitting
def test_split_batch_equals_the_sum_over_its_halves(pa, dev):
    from phoenix_amd import _lib
    N, H, B = 700, 40, 6000      # 4096 + 1904 rows: two launches, the second ragged
    lib = _lib.load()
    launches = lib.phx_debug_backprop_launches(N, H, B, 5, _lib.METHODS["rk4"])
    assert launches >= 2, "the batch must be large enough for the chunk driver to split it"
    p = rand_params(N, H, seed=11, std=0.05)
    net = make_net(pa, dev, p)
    r = np.random.RandomState(12)
    y0 = torch.from_numpy(r.rand(B, N).astype(np.float32)).to(dev)
    t = torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0], device=dev)
    G = torch.from_numpy((r.randn(5, B, N) / (B * N)).astype(np.float32)).to(dev)
    for h in (None, 0.75):
        whole = run_odeint(pa, net, y0, t, G, "rk4", h)
        lo = run_odeint(pa, net, y0[:B // 2], t, G[:, :B // 2].contiguous(), "rk4", h)
        hi = run_odeint(pa, net, y0[B // 2:], t, G[:, B // 2:].contiguous(), "rk4", h)
        for k in KEYS:
            e = relerr(whole["grad_" + k], lo["grad_" + k].astype(np.float64) + hi["grad_" + k])
            print("split h=%s %s %.2e (launches %d)" % (h, k, e, launches))
            assert e < TOL_FIXED, (h, k, e)
        # (the halves plan other gene tiles than the chunks of the whole batch: other summation orders, same bar)
        assert relerr(whole["grad_y0"], np.concatenate([lo["grad_y0"], hi["grad_y0"]])) < TOL_FIXED


# ------------------------------------------------------------------------------------------ 6: refusals at the call site
def test_refusals_come_from_the_call(pa, dev, g18):
    from phoenix_amd import engine
    net = make_net(pa, dev, sub(g18, "p_"))
    y0 = torch.from_numpy(g18["y0_batch"]).to(dev).requires_grad_(True)
    t = torch.from_numpy(g18["t5"]).to(dev)
    before = (dict(engine._ws_last), {k: v.data_ptr() for k, v in engine._ws_cache.items()})
    # 9 time units at h = 1e-6: nine million grid steps x 5 x 40 x 4 bytes, merely large
    with pytest.raises(RuntimeError, match="BACKPROP_MAX_CHECKPOINT_BYTES"):
        pa.odeint(net, y0, t, method="rk4", options={"step_size": 1e-6})
    assert before == (dict(engine._ws_last), {k: v.data_ptr() for k, v in engine._ws_cache.items()}), "nothing was launched"
    wide = pa.ODENet(dev, 64, neurons=300)
    with pytest.raises(RuntimeError, match="H = 128"):
        pa.odeint(wide, torch.rand(3, 1, 64, device=dev, requires_grad=True), t, method="rk4")
    mid = pa.ODENet(dev, 64, neurons=200)      # 128 < H <= 256: refused at the call as well
    with pytest.raises(RuntimeError, match="H = 128"):
        pa.odeint(mid, torch.rand(3, 1, 64, device=dev, requires_grad=True), t, method="euler")
    assert before == (dict(engine._ws_last), {k: v.data_ptr() for k, v in engine._ws_cache.items()})
    with torch.no_grad():                      # forward-only callers are unaffected
        assert pa.odeint(mid, torch.rand(3, 1, 64, device=dev), t, method="euler").shape == (5, 3, 1, 64)


# ------------------------------------------------------------------------------------------ 7: status modes
def test_forward_assertion_comes_out_of_backward(pa, dev, g18):
    from phoenix_amd import engine
    net = make_net(pa, dev, sub(g18, "p_"))
    y0 = torch.from_numpy(g18["y0_batch"]).to(dev)
    t = torch.from_numpy(g18["t5"]).to(dev)
    o = {"step_size": 0.5, "max_num_steps": 17}      # the grid has 18 steps
    yr = y0.clone().requires_grad_(True)
    sol = pa.odeint(net, yr, t, method="rk4", options=o)
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        sol.sum().backward()
    engine.set_status_mode("deferred")
    try:
        yr = y0.clone().requires_grad_(True)
        sol = pa.odeint(net, yr, t, method="rk4", options=o)
        sol.sum().backward()                         # nothing is read here
        with pytest.raises(AssertionError, match="max_num_steps exceeded"):
            engine.check_pending_status(wait=True)
    finally:
        engine.set_status_mode("immediate")
    yr = y0.clone().requires_grad_(True)
    pa.odeint(net, yr, t, method="rk4", options={"step_size": 0.5, "max_num_steps": 18}).sum().backward()
    assert torch.isfinite(yr.grad).all()


def test_graphed_step_records_and_replays(pa, dev, g18):
    """a step built on odeint(method="rk4") inside GraphedStep: the replay computes what the eager step computes"""
    from phoenix_amd.graphs import GraphedStep
    net = make_net(pa, dev, sub(g18, "p_"))
    y0 = torch.from_numpy(g18["y0_batch"]).to(dev)
    t = torch.from_numpy(g18["t5"]).to(dev)
    G = torch.from_numpy(g18["G/t5/batch"]).to(dev)
    want = run_odeint(pa, net, y0, t, G, "rk4", None)

    def step():
        for p in net.parameters():
            if p.grad is not None:
                p.grad.zero_()
        (pa.odeint(net, y0, t, method="rk4") * G).sum().backward()

    zero_grads(net)
    gs = GraphedStep(step)
    gs()
    gs.check_status()
    torch.cuda.synchronize()
    got = grads_of(net)
    for k in KEYS:
        assert relerr(got[k], want["grad_" + k]) < 1e-6, k


def test_launch_count_is_one_solve_kernel_per_chunk(pa, dev):
    from phoenix_amd import _lib
    lib = _lib.load()
    assert lib.phx_debug_backprop_kernel_m(350, 40, 1024, 5, _lib.METHODS["rk4"]) == 5
    assert lib.phx_debug_backprop_launches(350, 40, 1024, 5, _lib.METHODS["rk4"]) == 1
    assert lib.phx_debug_backprop_kernel_m(350, 200, 1024, 5, _lib.METHODS["rk4"]) == 0
