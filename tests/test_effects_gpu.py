"""The effects matrix and the state Jacobian on the MI355X: phx_effects_matrix (through the C ABI, via phoenix_amd.engine)
against the float64 evaluation of the formulas of include/phoenix_hip.h on the same float32 inputs, and
`effects_matrix` / `jacobian_matrix` against the reference's own results (golden G20, tests/golden/make_golden_effects.py).

The kernel bar is derived, not measured (test_effects_cpu.kernel_bound): entry by entry
    |got - ref64| <= (2H + 16 + B) 2^-24 A[i, j]
with A the same formula on absolute values (B = 0 for the effects matrix), and exactly 0 where A is 0.  The analysis
outputs are held to the 2e-5 max-norm bar of tests/test_influence_gpu.py (ph is then a length-N float32 contraction).
Every test prints the figures it measured before it asserts (run with -s to see them).
Measured on an MI355X (test_kernel_against_float64, worst |error| / bound over the three modes): (33, 1, 1) 0.22, (37, 5, 3)
0.14, (97, 7, 5) 0.10, (350, 40, 6) 0.05, (515, 200, 2) 0.012, (700, 128, 2) 0.018, last 70 rows of (11165, 40, 2) 0.053 and
of (14691, 200, 1) 0.014.  G20: effects 0.047 of twice the bound, both Jacobian means 5.2e-8 (the reference's own float32
Jacobians 3.6e-8).  Memory test: kernel 16 907 776 bytes, torch formulation 117 832 704, budget 32 000 000."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub
from test_effects_cpu import closed_form, kernel_bound
from test_gpu_parity import make_net, rand_params

pytestmark = pytest.mark.gpu

TOL = 2e-5      # the bar of the analysis outputs (tests/test_influence_gpu.py)
MODES = ("effects", "mean", "mean_abs")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def states(N, B, seed):
    """float32 states in [-0.2, 1.2], one entry exactly 0.5"""
    y = (np.random.RandomState(seed).rand(B, N) * 1.4 - 0.2).astype(np.float32)
    y[B // 2, min(7, N - 1)] = 0.5
    assert y.min() >= -0.2 and y.max() <= 1.2
    return y


def case(pa, dev, N, H, B, seed=None, p=None):
    """(p numpy, net, engine Params, y numpy, y device, ph device float32)"""
    from phoenix_amd import engine
    from phoenix_amd.odenet import params_of
    if p is None:
        p = rand_params(N, H, seed=N + H if seed is None else seed, std=0.6 / np.sqrt(N))
        assert (p["g"] < 0).any()
    net = make_net(pa, dev, p)
    params = engine.params_cached(*params_of(net))
    y = states(N, B, seed=N + B)
    yd = torch.from_numpy(y).to(dev)
    s = yd - 0.5
    ph = torch.exp(torch.addmm(params.bp, torch.log1p(s / (1 + s.abs())), params.Wp.t()))
    return p, net, params, y, yd, ph


def check(tag, got, ref, A, H, B):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, bound = np.abs(got - ref), kernel_bound(H, B, A)
    pos = A > 0
    worst = float(np.max(err[pos] / bound[pos]))
    print("%s: worst |error| / bound %.4f, max-norm relative error %.3e, %d entries with A = 0"
          % (tag, worst, float(err.max() / np.abs(ref).max()), int((~pos).sum())))
    assert np.all(got[~pos] == 0)
    assert np.all(err <= bound)


# --------------------------------------------------------------------------- 1. the kernel against float64
@pytest.mark.parametrize("N,H,B,tail", [(33, 1, 1, None), (37, 5, 3, None), (97, 7, 5, None), (350, 40, 6, None),
                                        (515, 200, 2, None), (700, 128, 2, None), (11165, 40, 2, 70), (14691, 200, 1, 70)])
def test_kernel_against_float64(pa, dev, N, H, B, tail):
    from phoenix_amd import engine
    p, _, params, y, yd, ph = case(pa, dev, N, H, B)
    rows = None if tail is None else (N - tail, N)
    phn = ph.cpu().numpy()
    for mode in MODES:
        ref, A = closed_form(p, mode, y=y, ph=phn, rows=rows)
        got = engine.effects_matrix(params, mode, y=yd, ph=ph, rows=rows)
        assert got.dtype == torch.float32 and got.is_cuda
        check("N=%d H=%d B=%d rows=%s %s" % (N, H, B, rows, mode), got, ref, A, H, 0 if mode == "effects" else B)


# --------------------------------------------------------------------------- 2. row ranges and repeatability
@pytest.mark.parametrize("N,H,B", [(97, 7, 5), (350, 40, 6)])
def test_row_ranges_agree_bit_for_bit(pa, dev, N, H, B):
    from phoenix_amd import engine
    _, _, params, _, yd, ph = case(pa, dev, N, H, B)
    for mode in MODES:
        full = engine.effects_matrix(params, mode, y=yd, ph=ph)
        again = engine.effects_matrix(params, mode, y=yd, ph=ph)
        chunks = torch.cat([engine.effects_matrix(params, mode, y=yd, ph=ph, rows=(r, min(r + 37, N)))
                            for r in range(0, N, 37)])
        part = engine.effects_matrix(params, mode, y=yd, ph=ph, rows=(13, 50))
        same = [torch.equal(again, full), torch.equal(chunks, full), torch.equal(part, full[13:50])]
        print("N=%d %s: repeat / chunks of 37 / rows [13, 50) identical to the full matrix: %s" % (N, mode, same))
        assert all(same)
        assert full.view(torch.int32).ne(0).any()


# --------------------------------------------------------------------------- 3. the diagonal term
@pytest.mark.parametrize("rows", [None, (13, 50), (64, 97), (5, 6)])
def test_diagonal_belongs_to_the_global_row(pa, dev, rows):
    """Ws = Wp = 0: J_b = -relu(g_j) delta_ij for every state, so both means are exact"""
    from phoenix_amd import engine
    N, H, B = 97, 7, 3
    p = rand_params(N, H, seed=5, std=0.6 / np.sqrt(N))
    p["Ws"][:], p["Wp"][:] = 0, 0
    _, _, params, _, yd, ph = case(pa, dev, N, H, B, p=p)
    r0, r1 = rows or (0, N)
    want = torch.zeros((r1 - r0, N), device=dev)
    idx = torch.arange(r0, r1, device=dev)
    want[idx - r0, idx] = torch.relu(torch.from_numpy(p["g"]).to(dev))[idx]
    mean = engine.effects_matrix(params, "mean", y=yd, ph=ph, rows=rows)
    mabs = engine.effects_matrix(params, "mean_abs", y=yd, ph=ph, rows=rows)
    print("rows %s: diagonal of mean %s ..., of mean_abs %s ..." % (rows, mean[idx - r0, idx][:3].tolist(),
                                                                 mabs[idx - r0, idx][:3].tolist()))
    assert torch.equal(mean, -want) and torch.equal(mabs, want)


def test_one_state_mean_abs_is_the_absolute_mean(pa, dev):
    from phoenix_amd import engine
    for N, H in ((97, 7), (350, 40)):
        _, _, params, _, yd, ph = case(pa, dev, N, H, 1)
        mean = engine.effects_matrix(params, "mean", y=yd, ph=ph)
        mabs = engine.effects_matrix(params, "mean_abs", y=yd, ph=ph)
        print("N=%d B=1: mean_abs == |mean| bit for bit: %s" % (N, torch.equal(mabs, mean.abs())))
        assert torch.equal(mabs, mean.abs()) and bool((mean < 0).any())


# --------------------------------------------------------------------------- 4. non-finite inputs
def test_non_finite_inputs_propagate(pa, dev):
    from phoenix_amd import engine
    N, H, B = 97, 7, 5
    p, _, params, _, yd, ph = case(pa, dev, N, H, B)
    b, i = 3, 70
    bad = yd.clone()
    bad[b, i] = float("nan")
    for mode in ("mean", "mean_abs"):
        for rows in (None, (60, 90)):
            out = engine.effects_matrix(params, mode, y=bad, ph=ph, rows=rows)
            nan_rows = torch.isnan(out).any(dim=1).nonzero().reshape(-1).tolist()
            print("NaN in y[%d, %d], %s rows %s: rows with NaN %s" % (b, i, mode, rows, nan_rows))
            assert nan_rows == [i - (rows[0] if rows else 0)]
            assert bool(torch.isnan(out[nan_rows[0]]).all())
            assert bool(torch.isfinite(out).sum() == out.numel() - N)
    h = 4
    bad = ph.clone()
    bad[1, h] = float("inf")
    out = engine.effects_matrix(params, "mean_abs", y=yd, ph=bad)
    reach = (np.abs(p["Wp"][h])[:, None] * np.abs(p["Wa"][:, H + h])[None, :] * np.maximum(p["g"], 0)[None, :]) != 0
    finite = torch.isfinite(out).cpu().numpy()
    print("inf in ph[1, %d]: %d of %d entries non-finite, %d must be" % (h, int((~finite).sum()), finite.size, int(reach.sum())))
    assert reach.sum() > 0 and not finite[reach].any()


def test_a_nan_multiplier_reaches_its_column_only(pa, dev):
    """torch.relu, which the reference scales with, keeps a NaN multiplier: column j is NaN, every other column as before"""
    from phoenix_amd import engine
    N, H, B = 97, 7, 3
    p = rand_params(N, H, seed=N + H, std=0.6 / np.sqrt(N))
    _, net_clean, clean, _, yd, ph = case(pa, dev, N, H, B, p=p)      # (both networks stay alive: the layout cache
    want = {m: engine.effects_matrix(clean, m, y=yd, ph=ph) for m in MODES}
    j = 41
    p["g"][j] = np.nan
    _, net_nan, params, _, _, _ = case(pa, dev, N, H, B, p=p)       #  keys on the parameter tensors' storage)
    keep = [c for c in range(N) if c != j]
    for mode in MODES:
        out = engine.effects_matrix(params, mode, y=yd, ph=ph)
        print("NaN in g[%d], %s: NaN entries %d (column holds %d)" % (j, mode, int(torch.isnan(out).sum()), N))
        assert bool(torch.isnan(out[:, j]).all()) and torch.equal(out[:, keep], want[mode][:, keep])
    assert net_clean is not net_nan


def test_buffers_of_another_dtype_are_refused(pa, dev):
    from phoenix_amd import engine
    N, H, B = 97, 7, 3
    _, net, params, _, yd, ph = case(pa, dev, N, H, B)
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            engine.effects_matrix(params, "effects", out=torch.zeros((N, N), dtype=dtype, device=dev))
        with pytest.raises(TypeError, match="float32"):
            pa.effects_matrix(net, rows=(3, 9), out=torch.zeros((6, N), dtype=dtype, device=dev))
    with pytest.raises(TypeError, match="float32"):
        engine.effects_matrix(params, "mean", y=yd.to(torch.int32), ph=ph)
    with pytest.raises(TypeError, match="float32"):
        engine.effects_matrix(params, "mean", y=yd, ph=ph.to(torch.int32))


# --------------------------------------------------------------------------- 5. the reference's own results
def test_golden_effects_and_jacobians(pa, dev):
    g = load_golden("g20_effects")
    p = sub(g, "p_")
    H, N = p["Ws"].shape
    net = make_net(pa, dev, p)
    _, A = closed_form(p, "effects")
    got = pa.effects_matrix(net).cpu().numpy()
    err, bound = np.abs(got.astype(np.float64) - g["effects"]), 2 * kernel_bound(H, 0, A)
    print("G20 effects: worst |got - reference| / (2 x bound) = %.4f" % float(np.max(err[A > 0] / bound[A > 0])))
    assert np.all(err <= bound) and np.all(got[A == 0] == 0)
    y = torch.from_numpy(g["y"]).to(dev)
    for reduce, ref, ref32 in (("mean", g["jac64"].mean(0), g["jac32"].astype(np.float64).mean(0)),
                               ("mean_abs", np.abs(g["jac64"]).mean(0), np.abs(g["jac32"].astype(np.float64)).mean(0))):
        got = pa.jacobian_matrix(net, y, reduce=reduce).cpu().numpy()
        e, e32 = relerr(got, ref), relerr(ref32, ref)
        print("G20 jacobian %s: max-norm relative error %.3e (the reference's own float32 Jacobians: %.3e)" % (reduce, e, e32))
        assert e < TOL
        assert np.all(got[:, p["g"] <= 0] == 0)


# --------------------------------------------------------------------------- 6. the Python surface
def test_python_surface(pa, dev):
    N, H, B = 97, 7, 5
    _, net, _, _, yd, _ = case(pa, dev, N, H, B)
    eff = pa.effects_matrix(net)
    jac = pa.jacobian_matrix(net, yd)
    for x in (eff, jac):
        assert x.shape == (N, N) and x.dtype == torch.float32 and x.device == dev
    assert torch.equal(jac, pa.jacobian_matrix(net, yd, reduce="mean_abs"))
    assert not torch.equal(jac, pa.jacobian_matrix(net, yd, reduce="mean"))
    # rows= is the slice of the full result; out= is written in place
    assert torch.equal(pa.effects_matrix(net, rows=(20, 31)), eff[20:31])
    assert torch.equal(pa.jacobian_matrix(net, yd, rows=(20, 31)), jac[20:31])
    buf = torch.full((11, N), float("nan"), device=dev)
    assert pa.effects_matrix(net, rows=(20, 31), out=buf) is buf and torch.equal(buf, eff[20:31])
    buf.fill_(float("nan"))
    assert pa.jacobian_matrix(net, yd, rows=(20, 31), out=buf) is buf and torch.equal(buf, jac[20:31])
    with pytest.raises(ValueError, match="out"):
        pa.effects_matrix(net, out=buf)
    # [B, 1, N] states are the same states
    assert torch.equal(pa.jacobian_matrix(net, yd.reshape(B, 1, N)), jac)
    with pytest.raises(ValueError, match="y must be"):
        pa.jacobian_matrix(net, yd[:, :50])
    # nothing is recorded for autograd
    assert not eff.requires_grad and not jac.requires_grad
    # an in-place parameter update is seen by the next call
    with torch.no_grad():
        net.net_sums.linear_out.weight[2, 30] += 1.0
    eff2, jac2 = pa.effects_matrix(net), pa.jacobian_matrix(net, yd)
    changed = (eff2 != eff).any(dim=1).nonzero().reshape(-1).tolist()
    print("after bumping Ws[2, 30]: rows of the effects matrix that changed %s" % changed)
    assert changed == [30] and not torch.equal(jac2, jac)
    assert torch.equal(jac2[:30], jac[:30]) and torch.equal(jac2[31:], jac[31:])


# --------------------------------------------------------------------------- 7. no N x N temporaries
def _torch_mean_abs(params, y, ph):
    """the per-state torch formulation of the same matrix"""
    H, N = params.H, params.N
    r = torch.relu(params.g)
    s = y - 0.5
    da = 1 / (1 + s.abs()) ** 2
    dl = torch.where(s < 0, 1 / (1 + s.abs()), 1 / ((1 + s) * (1 + 2 * s)))
    S = params.Ws.t() @ params.WaT[:H]
    acc = torch.zeros((N, N), device=y.device)
    eye = torch.eye(N, device=y.device)
    for b in range(y.shape[0]):
        Q = (params.Wp * ph[b][:, None]).t() @ params.WaT[H:]
        acc += (r * (da[b][:, None] * S + dl[b][:, None] * Q - eye)).abs()
    return acc / y.shape[0]


def test_the_jacobian_mean_allocates_its_result_only(pa, dev):
    """N = 2000, H = 40, 16 states: beyond the steady state (laid-out parameters) `jacobian_matrix` holds its [N, N] result
    and [B, N]-sized plumbing; one more N x N buffer would already cross the line that the torch formulation crosses"""
    N, H, B = 2000, 40, 16
    _, net, params, _, yd, ph = case(pa, dev, N, H, B)
    budget = 2 * N * N * 4
    grown = {}
    for name, fn in (("kernel", lambda: pa.jacobian_matrix(net, yd, reduce="mean_abs")),
                     ("torch", lambda: _torch_mean_abs(params, yd, ph))):
        first = fn()                                        # steady state: parameter layout, library handles
        torch.cuda.synchronize()
        if name == "kernel":
            e = relerr(first.cpu().numpy(), _torch_mean_abs(params, yd, ph).cpu().numpy())
            print("kernel vs torch formulation at N=2000: max-norm relative difference %.3e" % e)
            assert e < TOL
        del first
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = fn()
        torch.cuda.synchronize()
        grown[name] = torch.cuda.max_memory_allocated() - base
        del res
    print("peak growth of mean |J| at N=2000, B=16: kernel %d bytes, torch formulation %d bytes, budget %d"
          % (grown["kernel"], grown["torch"], budget))
    assert grown["kernel"] < budget
    assert grown["torch"] > budget
