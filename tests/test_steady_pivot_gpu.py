"""GPU tests of the two dense solves of the steady-state family on systems that exchange rows: k_st_solve (engine.steady_solve)
and k_sr_inverse (engine.steady_inverse) against float64 of the same float32 inputs under derived bars.  The inputs, the truth,
the bars, the mirror of the documented algorithm (which decides the info codes) and the proof that the bars bite are in
tests/test_steady_pivot_cpu.py; nothing here is measured from the device.

  each system    every case of `cases()` (exact P D, dense and its transpose, the strongly coupled models and their transposes;
                 n = 2 .. 512) through both kernels: info 0, every entry under its bar, the exact systems bit for bit, and
                 Z w consistent with x under the sum of the two bars.
  info codes     D[k] = 0 in P D at n = 130 (k + 1, zeros); NaN, +Inf, -Inf below, on and above the diagonal of an early
                 and a late column (the mirror's code, zeros); a solution beyond the float range (-1, zeros).
  neighbours     a batch of [dense, singular, exact, NaN, float range, dense^T]: every state has the bits of the state solved
                 alone, at another position, and in a second call.
  end to end     (70, 97, 3) with Wa x 3 (fixed points in -3.5 .. 5.2, the transposed systems exchange rows there):
                 steady_states(differentiable=True) and steady_state_response held exactly as tests/test_steady_adjoint_gpu.py
                 and tests/test_steady_response_gpu.py hold their own shapes; the count of kernel_truth's roundings for this
                 range is in the CPU file.

Measured on the MI355X, worst error / bar of x, of Z, and of Z w against x (every exact system equal in every bit):
    n     dense               dense T             model x3            model x3 T          model x8            model x8 T
    2     0.396 0.412 0.368   0.621 0.412 0.373
    4     0.560 0.920 0.309   0.795 0.920 0.493
    64    0.830 0.978 0.298   0.926 0.978 0.195
    66    0.757 0.988 0.243   0.951 0.988 0.416
    112                                           0.910 0.988 0.267   0.907 0.989 0.281   0.939 0.981 0.213   0.953 0.981 0.310
    128   0.859 0.930 0.196   0.810 0.928 0.158
    130   0.861 0.959 0.167   0.836 0.963 0.179
    194   0.502 0.845 0.070   0.730 0.844 0.099   0.966 0.992 0.232   0.937 0.992 0.219   0.796 0.913 0.164   0.812 0.910 0.146
    400                                           0.936 0.984 0.152   0.959 0.984 0.212   0.231 0.537 0.026   0.238 0.516 0.037
    512   0.069 0.254 0.004   0.061 0.256 0.006
(up to n ~ 200 the bar is little more than the one rounding to float, u |x|, which a correctly rounded entry can all but
reach: the CPU mirror gives the same 0.98 for Z).  End to end: 8 steps, y* in -3.52 .. 5.22, exchanges (S, S^T) (2, 1), (0, 1),
(1, 1); gradients |device - ref64| 6.5e-7 .. 1.7e-5 under bounds of 9.3e-6 .. 1.1e-4; response 3.0e-6 of its bound at most.
The float range: before the fix both kernels compared the double result with the double range, so the n = 6 system came
back with info 0, x = (inf, inf, inf, inf, inf, 16777216) and the Z row (16777216, inf, inf, inf, inf, inf); now info -1
and zeros."""
import collections

import numpy as np
import pytest
import torch

from test_gpu_parity import make_net
from test_steady_adjoint_gpu import FIELDS, back64, device_grads, pgrads64
from test_steady_adjoint_gpu import gamma as gamma32
from test_steady_cpu import moving, parts64
from test_steady_pivot_cpu import (END_TO_END, INFO_N, MODEL_SHAPES, SIZES, Y_RANGE, cases, exchanges, float_range_system,
                                   judge, mirror, neighbours, non_finite_systems, singular_systems, strong_model)
from test_steady_response_gpu import INPUTS, end_to_end_bound, engine_params, hold

pytestmark = pytest.mark.gpu
ALL_N = sorted(set(SIZES) | set(2 * H for _, H, _ in MODEL_SHAPES))     # every n of `cases()`


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def both(dev, S, w):
    """(x, Z, info_x, info_Z) as numpy of a batch S [B, n, n], w [B, n] of numpy float32"""
    from phoenix_amd import engine
    tS, tw = torch.from_numpy(np.ascontiguousarray(S)).to(dev), torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    x, ix = engine.steady_solve(tS, tw)
    Z, iZ = engine.steady_inverse(tS)
    assert x.dtype == Z.dtype == torch.float32 and ix.dtype == iZ.dtype == torch.int32
    assert x.shape == tw.shape and Z.shape == tS.shape and ix.shape == iZ.shape == (len(S),)
    return x.cpu().numpy(), Z.cpu().numpy(), ix.cpu().numpy(), iZ.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("n", ALL_N)
def test_each_system_against_the_truth_and_the_bar(dev, n):
    group = [c for c in cases() if c.n == n]
    x, Z, ix, iZ = both(dev, np.stack([c.S for c in group]), np.stack([c.w for c in group]))
    worst, failures = collections.defaultdict(lambda: (0.0, 0.0, 0.0)), []
    for b, c in enumerate(group):
        failed, w = judge(c, x[b], Z[b], int(ix[b]), int(iZ[b]))
        if failed:
            failures.append((c.name, failed))
        if w is not None:
            worst[c.cls] = tuple(max(p, q) for p, q in zip(worst[c.cls], w))
    print("n = %d: worst error / bar (x, Z, Z w - x) %s" % (n, {k: "%.3f %.3f %.3f" % v for k, v in worst.items()}))
    assert not failures, failures


def test_info_codes(dev):
    sing, bad = singular_systems(), non_finite_systems()
    S = np.stack([s[1] for s in sing] + [s[1] for s in bad] + [float_range_system(INFO_N)[0]])
    w = np.stack([s[2] for s in sing] + [s[2] for s in bad] + [float_range_system(INFO_N)[1]])
    want = [s[3] + 1 for s in sing] + [mirror(s[1], s[2])[2] for s in bad] + [-1]
    x, Z, ix, iZ = both(dev, S, w)
    print("info: solve %s, inverse %s, expected %s" % (ix.tolist(), iZ.tolist(), want))
    assert ix.tolist() == want and iZ.tolist() == want
    assert not x.any() and not Z.any() and same_bits(x, np.zeros_like(x)) and same_bits(Z, np.zeros_like(Z))
    # the float range at n = 6: finite in double (7.3e193 .. 1.7e7), not as float
    S6, w6 = float_range_system(6)
    x, Z, ix, iZ = both(dev, S6[None], w6[None])
    print("float range, n = 6: info %d, %d, x %s" % (ix[0], iZ[0], x[0].tolist()))
    assert ix.tolist() == [-1] and iZ.tolist() == [-1] and not x.any() and not Z.any()


def test_neighbours(dev):
    """a state's bits do not depend on the batch, on its position in it, or on the call"""
    states = neighbours()
    S, w = np.stack([s[1] for s in states]), np.stack([s[2] for s in states])
    x, Z, ix, iZ = both(dev, S, w)
    assert ix.tolist() == iZ.tolist() and [int(np.sign(i)) for i in ix] == [0, 1, 0, 1, -1, 0], ix.tolist()
    again = both(dev, S, w)
    order = [3, 5, 0, 4, 2, 1]
    moved = both(dev, S[order], w[order])
    for got, ref in zip(again, (x, Z, ix, iZ)):
        assert same_bits(got, ref)
    for got, ref in zip(moved, (x, Z, ix, iZ)):
        assert same_bits(got, ref[order])
    for b, (name, Sb, wb) in enumerate(states):
        alone = both(dev, Sb[None], wb[None])
        for got, ref in zip(alone, (x, Z, ix, iZ)):
            assert same_bits(got, ref[b:b + 1]), name
    # the healthy states beside the others are solved: the first and the last are the dense system and its transpose
    for b, name in ((0, "dense %d" % INFO_N), (5, "dense T %d" % INFO_N), (2, "exact cyclic %d" % INFO_N)):
        c = next(c for c in cases() if c.name == name)
        assert judge(c, x[b], Z[b], int(ix[b]), int(iZ[b]))[0] is None, name


def test_steady_solve_takes_views_and_checks_its_arguments(dev):
    from phoenix_amd import engine
    c = next(c for c in cases() if c.name == "dense %d" % INFO_N)
    S, w = torch.from_numpy(np.stack([c.S, c.S.T.copy()])).to(dev), torch.from_numpy(np.stack([c.w, c.w])).to(dev)
    view = S.transpose(1, 2)
    assert not view.is_contiguous()
    x, info = engine.steady_solve(view, w)
    x2, info2 = engine.steady_solve(view.contiguous(), w)
    assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(info, info2) and not info.any()
    plain = engine.steady_solve(S, w)[0]
    assert torch.equal(x[0], plain[1]) and torch.equal(x[1], plain[0]) and not torch.equal(x, plain)
    # a strided right-hand side too
    wide = torch.stack([w, w], dim=2)[:, :, 0]
    assert not wide.is_contiguous() and torch.equal(engine.steady_solve(S, wide)[0], plain)
    for bad_S, bad_w in ((S[:, :, :-1], w), (S[:, :-1, :-1], w[:, :-1]), (S[0], w[0]), (S, w[:, :-1]), (S, w[:1]), (S, w[0])):
        with pytest.raises(ValueError, match="steady_solve"):
            engine.steady_solve(bad_S, bad_w)
    with pytest.raises(TypeError):
        engine.steady_solve(S.double(), w)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        engine.steady_solve(S, w.cpu())


# --------------------------------------------------------------------------- end to end, one strongly coupled shape
def test_end_to_end_on_a_model_whose_systems_exchange_rows(pa, dev):
    """(70, 97, 3) with Wa x 3.  The gradients: the bound of test_gradients_against_the_reference_at_the_devices_own_steady_
    states, 8 |ref32 - ref64| + gamma_B A.  The response: the bound of test_response_against_the_reference_at_the_devices_
    steady_states, end_to_end_bound; its kernel_truth counts 16 roundings for y in [0, 1), which holds on Y_RANGE by the
    count in tests/test_steady_pivot_cpu.py."""
    from phoenix_amd import engine
    N, H, B = END_TO_END
    p, y0, held = strong_model(N, H, B)
    net = make_net(pa, dev, p)
    for q in net.parameters():
        q.requires_grad_(True)
        q.grad = None
    y0t = torch.from_numpy(y0).to(dev).requires_grad_(True)
    out = pa.steady_states(net, y0t, clamp=held, differentiable=True)
    G = np.random.default_rng(1000 + N).standard_normal((B, N)).astype(np.float32)
    (out.y * torch.from_numpy(G).to(dev)).sum().backward()
    assert bool((out.status == 0).all()) and bool((pa.last_backward_info() == 0).all())
    ystar = out.y.detach().cpu().numpy()
    assert Y_RANGE[0] <= ystar.min() < -3 and 5 < ystar.max() <= Y_RANGE[1]
    m = moving(p, held, B).astype(np.float32)
    P, tm = engine_params(net), torch.from_numpy(m).to(dev)
    # from scipy on the device's own S: the systems of the adjoint exchanged rows
    S = engine.reduced_jacobian(P, out.y.detach(), tm)[0].cpu().numpy()
    counts = [(exchanges(S[b]), exchanges(S[b].T)) for b in range(B)]
    print("steps %s, y in %.2f .. %.2f, exchanges (S, S^T) %s" % (out.iterations.tolist(), ystar.min(), ystar.max(), counts))
    assert max(c[1] for c in counts) >= 1
    # the gradients
    r64 = pa.steady_states_adjoint_reference(p, ystar, G, clamp=held)
    r32 = pa.steady_states_adjoint_reference(p, ystar, G, clamp=held, dtype=np.float32)
    got = device_grads(net, y0t)
    _, A = pgrads64(p, ystar, r64.lam, r64.q, parts64(p, ystar)[4])
    A["y0"] = back64(p, ystar, None, G, r64.q, parts64(p, ystar)[4])[1]
    report = {}
    for k in ("y0",) + FIELDS:
        ref = getattr(r64, k)
        assert got[k].shape == ref.shape, k
        d32 = float(np.abs(getattr(r32, k).astype(np.float64) - ref).max())
        ddev = float(np.abs(got[k].astype(np.float64) - ref).max())
        report[k] = (ddev, d32, 8 * d32 + gamma32(B) * float(A[k].max()))
    print("gradients: |device - ref64|, |ref32 - ref64|, bound: %s" % {k: "%.2e %.2e %.2e" % v for k, v in report.items()})
    for k, v in report.items():
        assert v[0] <= v[2], (k, v)
    assert got["g"] is None or not got["g"].any()
    # the response
    for q in net.parameters():
        q.requires_grad_(False)
    st_y = out.y.detach()
    regs, worst = list(range(N)), {}
    for input in INPUTS:
        for reduce in ("mean_abs", "mean"):
            res = pa.steady_state_response(net, st_y, clamp=held, input=input, reduce=reduce, status=out.status)
            ref = pa.steady_state_response_reference(p, ystar, clamp=held, input=input, reduce=reduce)
            assert res.info.tolist() == ref.info.tolist() == [0] * B and res.response.shape == (N, N)
            out64, bar = end_to_end_bound(p, ystar, m, regs, input, reduce == "mean_abs")
            assert np.abs(out64 - ref.response).max() <= 1e-12          # the bound's own float64 chain is the reference's
            hold("%s %s" % (input, reduce), res.response, ref.response, bar, worst)
            sc = res.scores.cpu().numpy().astype(np.float64)
            sc_bar = (bar.sum(axis=1) + gamma32(N + 2) * (np.abs(ref.response) + bar).sum(axis=1)) / max(N - 1, 1)
            assert np.all(np.abs(sc - ref.scores) <= sc_bar)
    print("response: worst error / bound %s" % {n: "%.1e" % v for n, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
