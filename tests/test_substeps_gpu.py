"""options={"step_size": h} on euler / midpoint / rk4 against G17 (tests/golden/make_golden_substeps.py: the reference's
own odeint / odeint_adjoint with that option), forward and adjoint, on the MI355X.  Run with `-m gpu`.

Kernels with the sub-step loop: k1_solve_fwd, k1_solve_adj2 and k1_solve_adj.  The VALU engine (PHX_ENGINE=v0) does
not have it; dispatch skips it and forcing it is an error raised before any launch, never one step per interval."""

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub

pytestmark = pytest.mark.gpu

KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")
TOL_FIXED = 1e-5      # the project's fixed-grid bar (tests/test_gpu_parity.py)
HS = (0.5, 0.75, 0.125, 0.3)
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_substeps")


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


def check_case(pa, dev, func, net, g, c, y0, t, G, method, options, adjoint_options=None, tag=""):
    """solution and all seven gradients of sum(G * odeint_adjoint(...)) against the golden case `c`"""
    zero_grads(net)
    y0r = y0.clone().requires_grad_(True)
    sol = pa.odeint_adjoint(func, y0r, t, method=method, options=options, adjoint_options=adjoint_options)
    errs = {"sol": relerr(sol.detach().cpu().numpy(), c["sol"])}
    (sol * G).sum().backward()
    errs["grad_y0"] = relerr(y0r.grad.cpu().numpy(), c["grad_y0"])
    got = grads_of(net)
    for k in KEYS:
        errs["grad_" + k] = relerr(got[k], c["grad_" + k])
    print(tag, " ".join("%s=%.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < TOL_FIXED, (tag, k, e)


# ------------------------------------------------------------------------------------------ 1: every golden case
@pytest.mark.parametrize("yname", ["single", "batch"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("tname", ["t2", "t5", "t_dec"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_g17_forward_and_adjoint(pa, dev, g17, method, tname, h, yname):
    net = make_net(pa, dev, sub(g17, "p_"))
    c = sub(g17, "%s/%s/%r/%s/" % (method, tname, h, yname))
    y0 = torch.from_numpy(g17["y0_" + yname]).to(dev)
    t = torch.from_numpy(g17[tname]).to(dev)
    with torch.no_grad():
        sol = pa.odeint(net, y0, t, method=method, options={"step_size": h})
    assert sol.shape == c["sol"].shape
    e = relerr(sol.cpu().numpy(), c["sol"])
    print("odeint sol=%.2e" % e)
    assert e < TOL_FIXED
    G = torch.from_numpy(g17["G/%s/%s" % (tname, yname)]).to(dev)
    check_case(pa, dev, net, net, g17, c, y0, t, G, method, {"step_size": h}, tag="%s/%s/%r/%s" % (method, tname, h, yname))


def test_g17_step_size_as_a_tensor(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    with torch.no_grad():
        a = pa.odeint(net, y0, t, method="rk4", options={"step_size": 0.75})
        b = pa.odeint(net, y0, t, method="rk4", options={"step_size": torch.tensor(0.75, device=dev)})
    assert torch.equal(a, b)


def test_g17_adjoint_step_of_its_own(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    G = torch.from_numpy(g17["G/t5/batch"]).to(dev)
    check_case(pa, dev, net, net, g17, sub(g17, "adjstep/"), y0, t, G, "rk4", {"step_size": 0.5},
               adjoint_options={"step_size": 0.25}, tag="adjstep")


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_g17_float64_time_grid(pa, dev, g17, method):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5_64"]).to(dev)
    assert t.dtype == torch.float64
    with torch.no_grad():
        sol, nfe, ns = pa.odeint(net, y0, t, method=method, options={"step_size": 0.07}, return_stats=True)
    e = relerr(sol.cpu().numpy(), g17["f64/%s/sol" % method])
    print("f64 %s sol=%.2e nsteps=%s" % (method, e, ns.tolist()))
    assert e < TOL_FIXED
    assert ns.tolist() == [int(g17["nsteps/t5_64/0.07"])] * 5


# ------------------------------------------------------------------------------------------ 2: kernel selection
@pytest.mark.parametrize("np2", ["2", "4"])
@pytest.mark.parametrize("tname", ["t5", "t_dec"])
def test_g17_on_the_wave_pair_kernel_in_both_forms(pa, dev, g17, monkeypatch, tname, np2):
    monkeypatch.setenv("PHX_ADJ", "v2")
    monkeypatch.setenv("PHX_ADJ2_NP", np2)
    net = make_net(pa, dev, sub(g17, "p_"))
    t = torch.from_numpy(g17[tname]).to(dev)
    for yname in ("single", "batch"):
        y0 = torch.from_numpy(g17["y0_" + yname]).to(dev)
        G = torch.from_numpy(g17["G/%s/%s" % (tname, yname)]).to(dev)
        for h in HS:
            check_case(pa, dev, net, net, g17, sub(g17, "rk4/%s/%r/%s/" % (tname, h, yname)), y0, t, G, "rk4",
                       {"step_size": h}, tag="adj2 NP=%s %s/%r/%s" % (np2, tname, h, yname))


@pytest.mark.parametrize("tname", ["t5", "t_dec"])
def test_g17_on_the_first_generation_backward_kernel(pa, dev, g17, monkeypatch, tname):
    monkeypatch.setenv("PHX_ADJ", "v1")
    net = make_net(pa, dev, sub(g17, "p_"))
    from phoenix_amd import _lib
    assert _lib.load().phx_debug_adjoint_kernel_m(40, 6, 5, 5, _lib.CTRL_PER_TRAJECTORY, _lib.METHODS["rk4"] | 0x100) == 1
    t = torch.from_numpy(g17[tname]).to(dev)
    for method in ("euler", "midpoint", "rk4"):
        for yname in ("single", "batch"):
            y0 = torch.from_numpy(g17["y0_" + yname]).to(dev)
            G = torch.from_numpy(g17["G/%s/%s" % (tname, yname)]).to(dev)
            for h in HS:
                check_case(pa, dev, net, net, g17, sub(g17, "%s/%s/%r/%s/" % (method, tname, h, yname)), y0, t, G, method,
                           {"step_size": h}, tag="adj1 %s %s/%r/%s" % (method, tname, h, yname))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    check_case(pa, dev, net, net, g17, sub(g17, "adjstep/"), y0, torch.from_numpy(g17["t5"]).to(dev),
               torch.from_numpy(g17["G/t5/batch"]).to(dev), "rk4", {"step_size": 0.5}, adjoint_options={"step_size": 0.25},
               tag="adj1 adjstep")


class ReferenceShaped(torch.nn.Module):
    """a plain module with the structure of the reference's ODENet (net_sums / net_prods / net_alpha_combine .linear_out,
    gene_multipliers) that is not phoenix_amd.ODENet: recognised structurally (odenet.params_of), integrated by the engine.
    Its own forward is never called by the solvers."""

    class _Block(torch.nn.Module):
        def __init__(self, n_in, n_out, bias):
            super().__init__()
            self.linear_out = torch.nn.Linear(n_in, n_out, bias=bias)

    def __init__(self, p, dev):
        super().__init__()
        H, N = p["Ws"].shape
        self.net_sums = self._Block(N, H, True)
        self.net_prods = self._Block(N, H, True)
        self.net_alpha_combine = self._Block(2 * H, N, False)
        self.gene_multipliers = torch.nn.Parameter(torch.from_numpy(p["g"]).reshape(1, N).clone())
        with torch.no_grad():
            self.net_sums.linear_out.weight.copy_(torch.from_numpy(p["Ws"]))
            self.net_sums.linear_out.bias.copy_(torch.from_numpy(p["bs"]))
            self.net_prods.linear_out.weight.copy_(torch.from_numpy(p["Wp"]))
            self.net_prods.linear_out.bias.copy_(torch.from_numpy(p["bp"]))
            self.net_alpha_combine.linear_out.weight.copy_(torch.from_numpy(p["Wa"]))
        self.to(dev)

    def forward(self, t, y):
        raise AssertionError("the engine integrates this module; its forward is not used")


@pytest.mark.parametrize("yname", ["single", "batch"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("tname", ["t2", "t5", "t_dec"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_g17_through_the_structural_match(pa, dev, g17, method, tname, h, yname):
    net = ReferenceShaped(sub(g17, "p_"), dev)
    assert not isinstance(net, pa.ODENet)
    pa.odenet.params_of(net)
    c = sub(g17, "%s/%s/%r/%s/" % (method, tname, h, yname))
    y0 = torch.from_numpy(g17["y0_" + yname]).to(dev)
    t = torch.from_numpy(g17[tname]).to(dev)
    with torch.no_grad():
        e = relerr(pa.odeint(net, y0, t, method=method, options={"step_size": h}).cpu().numpy(), c["sol"])
    print("structural odeint sol=%.2e" % e)
    assert e < TOL_FIXED
    G = torch.from_numpy(g17["G/%s/%s" % (tname, yname)]).to(dev)
    check_case(pa, dev, net, net, g17, c, y0, t, G, method, {"step_size": h},
               tag="structural %s/%s/%r/%s" % (method, tname, h, yname))


def test_the_valu_engine_refuses_a_step_size_before_any_launch(pa, dev, g17, monkeypatch):
    """no kernel takes one step per interval in silence: the VALU kernels have no sub-step loop, so forcing them is an
    error -- raised by the forward call, not between the forward and the backward solve of a step"""
    monkeypatch.setenv("PHX_ENGINE", "v0")
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev).requires_grad_(True)
    t = torch.from_numpy(g17["t5"]).to(dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        pa.odeint_adjoint(net, y0, t, method="rk4", options={"step_size": 0.5})
    with torch.no_grad(), pytest.raises(RuntimeError, match="bad argument"):
        pa.odeint(net, y0, t, method="rk4", options={"step_size": 0.5})
    # ... while the same selection still serves the plain fixed grid
    sol = pa.odeint_adjoint(net, y0, t, method="rk4")
    sol.sum().backward()
    assert relerr(sol.detach().cpu().numpy(), load_golden("g3_fixed")["rk4/t5/batch/sol"]) < TOL_FIXED


def _rand_net(pa, dev, N, H, seed, std):
    r = np.random.RandomState(seed)
    g = r.rand(N).astype(np.float32)
    g[r.rand(N) < 0.1] *= -1
    p = {"Ws": (r.randn(H, N) * std).astype(np.float32), "bs": r.uniform(-.2, .2, H).astype(np.float32),
         "Wp": (r.randn(H, N) * std).astype(np.float32), "bp": r.uniform(-.2, .2, H).astype(np.float32),
         "Wa": (r.randn(N, 2 * H) * std).astype(np.float32), "g": g}
    y0 = torch.from_numpy((r.rand(5, 1, N) * 1.2).astype(np.float32)).to(dev)
    G = torch.from_numpy(r.randn(3, 5, 1, N).astype(np.float32)).to(dev)
    return make_net(pa, dev, p), y0, G


@pytest.mark.parametrize("shape", [(1100, 12, 0.02, 1), (96, 160, 0.03, 1), (350, 40, 0.05, 2)])
def test_shapes_of_every_backward_kernel_against_the_torch_stepper(pa, dev, shape):
    """(N, H, std, kernel): more than 32 gene tiles with a narrow hidden layer and H > 128 are k1_solve_adj's shapes, the
    third the wave-pair kernel's; forward and adjoint with a step size against generic.py's stepper (itself held to G17)"""
    from phoenix_amd import _lib
    N, H, std, kid = shape
    lib, m = _lib.load(), _lib.METHODS["rk4"] | 0x100
    assert lib.phx_debug_adjoint_kernel_m(N, H, 5, 3, _lib.CTRL_PER_TRAJECTORY, m) == kid
    assert lib.phx_debug_forward_kernel_m(N, H, 5, 3, _lib.CTRL_PER_TRAJECTORY, m) == 1
    net, y0, G = _rand_net(pa, dev, N, H, N + H, std)
    func = Wrapped(net)
    t = torch.tensor([0.0, 1.0, 2.2], device=dev)
    res = []
    for f in (net, func):
        zero_grads(net)
        yr = y0.clone().requires_grad_(True)
        sol = pa.odeint_adjoint(f, yr, t, method="rk4", options={"step_size": 0.3}, adjoint_options={"step_size": 0.25})
        (sol * G).sum().backward()
        res.append((sol.detach().cpu().numpy(), yr.grad.cpu().numpy(), grads_of(net)))
    errs = {"sol": relerr(res[0][0], res[1][0]), "grad_y0": relerr(res[0][1], res[1][1])}
    for k in KEYS:
        errs["grad_" + k] = relerr(res[0][2][k], res[1][2][k])
    print("N=%d H=%d" % (N, H), " ".join("%s=%.2e" % kv for kv in errs.items()))
    assert all(v < TOL_FIXED for v in errs.values()), errs


def test_odeint_calls_equals_the_separate_calls(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    y0s = torch.stack([y0, y0 * 0.5 + 0.1, y0[[4, 3, 2, 1, 0]]])
    t = torch.from_numpy(g17["t5"]).to(dev)
    got = pa.odeint_calls(net, y0s, t, method="rk4", options={"step_size": 0.75})
    with torch.no_grad():
        want = torch.stack([pa.odeint(net, y0s[k], t, method="rk4", options={"step_size": 0.75}) for k in range(3)])
    assert got.shape == (3, 5, 5, 1, 40) and torch.equal(got, want)
    assert relerr(got[0].cpu().numpy(), g17["rk4/t5/0.75/batch/sol"]) < TOL_FIXED


def test_max_num_steps_is_a_budget_of_grid_steps(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    with torch.no_grad():
        ok = pa.odeint(net, y0, t, method="rk4", options={"step_size": 0.5, "max_num_steps": 18})
        assert relerr(ok.cpu().numpy(), g17["rk4/t5/0.5/batch/sol"]) < TOL_FIXED
        with pytest.raises(AssertionError, match="max_num_steps exceeded"):
            pa.odeint(net, y0, t, method="rk4", options={"step_size": 0.5, "max_num_steps": 17})
        with pytest.raises(AssertionError, match="max_num_steps exceeded"):      # the default budget: no hour-long kernel
            pa.odeint(net, y0, t, method="rk4", options={"step_size": 1e-7})
    # the backward counts per interval (the longest of t5 at h = 0.5 has 8 steps)
    for budget, fails in ((18, False), (7, True)):
        yr = y0.clone().requires_grad_(True)
        sol = pa.odeint_adjoint(net, yr, t, method="rk4", options={"step_size": 4.5, "max_num_steps": budget},
                                adjoint_options={"step_size": 0.5})
        if fails:
            with pytest.raises(AssertionError, match="max_num_steps exceeded"):
                sol.sum().backward()
        else:
            sol.sum().backward()
            assert torch.isfinite(yr.grad).all()


# ------------------------------------------------------------------------------------------ 3: statistics
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("tname", ["t2", "t5", "t_dec"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_return_stats_counts_grid_steps(pa, dev, g17, method, tname, h):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17[tname]).to(dev)
    with torch.no_grad():
        _, nfe, ns = pa.odeint(net, y0, t, method=method, options={"step_size": h}, return_stats=True)
    n = int(g17["nsteps/%s/%r" % (tname, h)])
    assert ns.tolist() == [n] * 5 and nfe.tolist() == [STAGES[method] * n] * 5


def test_backward_counts_add_up_the_intervals(pa, dev, g17):
    from phoenix_amd import engine, _lib
    net = make_net(pa, dev, sub(g17, "p_"))
    pe = engine.params_cached(*pa.odenet.params_of(net))
    y2 = torch.from_numpy(g17["y0_batch"]).to(dev).reshape(5, 40).contiguous()
    for tname in ("t5", "t_dec"):
        t = torch.from_numpy(g17[tname]).to(dev)
        for h in HS:
            sol, st, _, _ = engine.solve_forward(pe, y2, t, "rk4", _lib.CTRL_SHARED, 1e-7, 1e-9, False, 2, step_size=h)
            _, _, st_b, nfe_b, ns_b = engine.solve_adjoint(pe, t, sol, torch.ones_like(sol), "rk4", _lib.CTRL_SHARED, 1e-7,
                                                           1e-9, False, 2, step_size=h)
            n = int(g17["nsteps_bwd/%s/%r" % (tname, h)].sum())
            assert int(st.max()) == 0 and int(st_b.max()) == 0
            assert ns_b.tolist() == [n] * 5 and nfe_b.tolist() == [4 * n] * 5, (tname, h)


# ------------------------------------------------------------------------------------------ 4: per-sample grids
def test_per_sample_grids_against_the_references_loop(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    c = sub(g17, "ps/")
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev).requires_grad_(True)
    t = torch.from_numpy(c["t"]).to(dev)
    G = torch.from_numpy(c["G"]).to(dev)
    sol = pa.odeint_per_sample(net, y0, t, method="rk4", options={"step_size": 0.25})
    errs = {"end": relerr(sol[1].detach().cpu().numpy(), c["end"])}
    (sol[1] * G[1]).sum().backward()
    errs["grad_y0"] = relerr(y0.grad.cpu().numpy(), c["grad_y0"])
    got = grads_of(net)
    for k in KEYS:
        errs["grad_" + k] = relerr(got[k], c["grad_" + k])
    print("per-sample", " ".join("%s=%.2e" % kv for kv in errs.items()))
    assert all(e < TOL_FIXED for e in errs.values()), errs
    with torch.no_grad():
        _, _, ns = pa.odeint(net, y0.detach(), t, method="rk4", options={"step_size": 0.25}, return_stats=True)
    assert ns.tolist() == c["nsteps"].tolist()


@pytest.mark.parametrize("B", [17, 33])
def test_padded_batches_equal_row_by_row_calls(pa, dev, g17, B):
    """mixed interval lengths (different step counts inside one workgroup), a batch that ends inside a tile"""
    net = make_net(pa, dev, sub(g17, "p_"))
    r = np.random.RandomState(B)
    y0 = torch.from_numpy((r.rand(B, 1, 40) * 1.2).astype(np.float32)).to(dev)
    t0 = r.rand(B).astype(np.float32)
    t = torch.from_numpy(np.stack([t0, t0 + 0.2 + 2.5 * r.rand(B).astype(np.float32),
                                   t0 + 3.0 + r.rand(B).astype(np.float32)], axis=1)).to(dev)
    G = torch.from_numpy(r.randn(3, B, 1, 40).astype(np.float32)).to(dev)
    zero_grads(net)
    yb = y0.clone().requires_grad_(True)
    sol = pa.odeint_per_sample(net, yb, t, method="rk4", options={"step_size": 0.3})
    (sol * G).sum().backward()
    gb, gp = yb.grad.clone(), grads_of(net)
    zero_grads(net)
    rows, grows = [], []
    for b in range(B):
        yr = y0[b].clone().requires_grad_(True)
        s = pa.odeint_adjoint(net, yr, t[b], method="rk4", options={"step_size": 0.3})
        (s * G[:, b]).sum().backward()
        rows.append(s.detach())
        grows.append(yr.grad)
    assert relerr(sol.detach().cpu().numpy(), torch.stack(rows, 1).cpu().numpy()) < TOL_FIXED
    assert relerr(gb.cpu().numpy(), torch.stack(grows).cpu().numpy()) < TOL_FIXED
    got = grads_of(net)
    for k in KEYS:
        assert relerr(gp[k], got[k]) < TOL_FIXED, k


# ------------------------------------------------------------------------------------------ 5: what the option is for
@pytest.mark.parametrize("yname", ["single", "batch"])
def test_sub_steps_are_closer_to_the_truth_than_one_step_per_interval(pa, dev, g17, yname):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_" + yname]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    truth = g17["truth64/" + yname]
    with torch.no_grad():
        fine = relerr(pa.odeint(net, y0, t, method="rk4", options={"step_size": 0.125}).cpu().numpy(), truth)
        coarse = relerr(pa.odeint(net, y0, t, method="rk4").cpu().numpy(), truth)
    print("distance to truth64: h=0.125 %.3e, one step per interval %.3e" % (fine, coarse))
    assert fine < coarse


# ------------------------------------------------------------------------------------------ 6: dopri5 ignores it
def test_dopri5_warns_and_returns_the_plain_result(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    with torch.no_grad():
        plain = pa.odeint(net, y0, t, method="dopri5")
        with pytest.warns(UserWarning, match="Unexpected arguments"):
            got = pa.odeint(net, y0, t, method="dopri5", options={"step_size": 0.5})
    assert torch.equal(plain, got)


# ------------------------------------------------------------------------------------------ 7: nothing else changed
def test_without_a_step_size_the_old_entry_points_are_what_runs(pa, dev, g17):
    import ctypes as C
    from phoenix_amd import engine, _lib
    g3 = load_golden("g3_fixed")
    net = make_net(pa, dev, sub(g3, "p_"))
    y0 = torch.from_numpy(g3["y0_batch"]).to(dev)
    t = torch.from_numpy(g3["t5"]).to(dev)
    G = torch.from_numpy(g3["rk4/t5/batch/G"]).to(dev)
    zero_grads(net)
    yr = y0.clone().requires_grad_(True)
    sol = pa.odeint_adjoint(net, yr, t, method="rk4")
    (sol * G).sum().backward()
    got = grads_of(net)
    with torch.no_grad():
        assert torch.equal(pa.odeint(net, y0, t, method="rk4"), sol.detach())
    # the same through phx_odeint / phx_odeint_adjoint_backward themselves
    lib = _lib.load()
    pe = engine.params_cached(*pa.odenet.params_of(net))
    y2 = y0.reshape(5, 40).contiguous()
    s2 = torch.empty((5, 5, 40), dtype=torch.float32, device=dev)
    stats = torch.empty((3, 5), dtype=torch.int32, device=dev)
    o = engine._opts("rk4", _lib.CTRL_SHARED, 1e-7, 1e-9, 0, 2, 0)
    ws, nb = engine._workspace(_lib.OP_ODEINT, 40, 6, 5, 5, dev)
    p_ = engine._p
    assert lib.phx_odeint(C.byref(pe.c), p_(y2), p_(t), 5, 5, C.byref(o), p_(s2), p_(stats[0]), p_(stats[1]), p_(stats[2]),
                          p_(ws), nb, engine._stream_ptr()) == 0
    assert torch.equal(s2.reshape(sol.shape), sol.detach())
    engine.forget_workspaces()
    adj = torch.empty((5, 40), dtype=torch.float32, device=dev)
    grads = pe.new_grads()
    ws, nb = engine._workspace(_lib.OP_ADJOINT, 40, 6, 5, 5, dev)
    Gc = G.reshape(5, 5, 40).contiguous()
    assert lib.phx_odeint_adjoint_backward(C.byref(pe.c), p_(t), 5, 5, C.byref(o), p_(s2), p_(Gc), p_(adj), C.byref(grads.c),
                                           p_(stats[0]), p_(stats[1]), p_(stats[2]), p_(ws), nb, engine._stream_ptr()) == 0
    engine.forget_workspaces()
    assert torch.equal(adj.reshape(yr.grad.shape), yr.grad)
    ref = grads.as_reference_layout(net.gene_multipliers.shape)
    for k, x in zip(KEYS, ref):
        assert np.array_equal(x.detach().cpu().numpy().reshape(got[k].shape), got[k]), k
        assert relerr(got[k], g3["rk4/t5/batch/grad_" + k]) < TOL_FIXED


# ------------------------------------------------------------------------------------------ 8: any other func
class Wrapped(torch.nn.Module):
    """the G17 net behind a module that is not recognised as an ODENet: the unfused torch stepper integrates it"""

    def __init__(self, net):
        super().__init__()
        self.inner = torch.nn.ModuleList([net])

    def forward(self, t, y):
        return self.inner[0](t, y)


@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("tname", ["t5", "t_dec"])
def test_generic_stepper_against_g17(pa, dev, g17, tname, h):
    net = make_net(pa, dev, sub(g17, "p_"))
    func = Wrapped(net)
    with pytest.raises(TypeError):
        pa.odenet.params_of(func)
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17[tname]).to(dev)
    G = torch.from_numpy(g17["G/%s/batch" % tname]).to(dev)
    c = sub(g17, "rk4/%s/%r/batch/" % (tname, h))
    with torch.no_grad():
        assert relerr(pa.odeint(func, y0, t, method="rk4", options={"step_size": h}).cpu().numpy(), c["sol"]) < TOL_FIXED
    check_case(pa, dev, func, net, g17, c, y0, t, G, "rk4", {"step_size": h}, tag="generic %s/%r" % (tname, h))


def test_generic_stepper_adjoint_step_of_its_own(pa, dev, g17):
    net = make_net(pa, dev, sub(g17, "p_"))
    y0 = torch.from_numpy(g17["y0_batch"]).to(dev)
    t = torch.from_numpy(g17["t5"]).to(dev)
    G = torch.from_numpy(g17["G/t5/batch"]).to(dev)
    check_case(pa, dev, Wrapped(net), net, g17, sub(g17, "adjstep/"), y0, t, G, "rk4", {"step_size": 0.5},
               adjoint_options={"step_size": 0.25}, tag="generic adjstep")


# ------------------------------------------------------------------------------------------ 9: full size
def _insilico(pa, dev):
    N, H, B = 350, 40, 1024
    g = torch.Generator(device="cpu").manual_seed(1234)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        net = pa.ODENet("cpu", N, neurons=H)
    with torch.no_grad():
        for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.05)
        net.gene_multipliers.copy_(torch.rand(1, N, generator=g))
    y0 = (torch.randn(B, 1, N, generator=g) * 0.15 + 0.5).clamp_(0.03, 1.07)
    G = torch.randn(5, B, 1, N, generator=g)
    t = torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0])
    return net.to(dev), y0.to(dev), t.to(dev), G.to(dev)


def test_full_size_forward_equals_the_dense_grid(pa, dev):
    net, y0, t, _ = _insilico(pa, dev)
    tb = t.repeat(y0.shape[0], 1)                        # per-sample rows, as the benchmark passes them
    dense = torch.arange(0.0, 9.5, 0.5, device=dev)
    with torch.no_grad():
        sub_ = pa.odeint(net, y0, tb, method="rk4", options={"step_size": 0.5})
        ref = pa.odeint(net, y0, dense.repeat(y0.shape[0], 1), method="rk4")[[0, 4, 6, 14, 18]]
        _, _, ns = pa.odeint(net, y0, tb, method="rk4", options={"step_size": 0.5}, return_stats=True)
    e = relerr(sub_.cpu().numpy(), ref.cpu().numpy())
    print("full size h=0.5 vs dense grid: %.2e" % e)
    assert e < TOL_FIXED and ns.tolist() == [18] * y0.shape[0]


def test_full_size_against_the_torch_stepper(pa, dev):
    net, y0, t, G = _insilico(pa, dev)
    func = Wrapped(net)
    tb = t.repeat(y0.shape[0], 1)
    with torch.no_grad():
        a = pa.odeint(net, y0, tb, method="rk4", options={"step_size": 0.75})
        b = pa.odeint(func, y0, t, method="rk4", options={"step_size": 0.75})
    e = relerr(a.cpu().numpy(), b.cpu().numpy())
    print("full size h=0.75 forward vs torch stepper: %.2e" % e)
    assert e < TOL_FIXED
    for h in (0.5, 0.75):
        res = []
        for f, tt in ((net, tb), (func, t)):
            zero_grads(net)
            yr = y0.clone().requires_grad_(True)
            (pa.odeint_adjoint(f, yr, tt, method="rk4", options={"step_size": h}) * G).sum().backward()
            res.append((yr.grad.cpu().numpy(), grads_of(net)))
        errs = {"grad_y0": relerr(res[0][0], res[1][0])}
        for k in KEYS:
            errs["grad_" + k] = relerr(res[0][1][k], res[1][1][k])
        print("full size h=%r adjoint vs torch stepper:" % h, " ".join("%s=%.2e" % kv for kv in errs.items()))
        assert all(v < TOL_FIXED for v in errs.values()), (h, errs)
