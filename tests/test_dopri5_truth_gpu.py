"""Every dopri5 kernel family against an fp64 truth captured from the reference (golden G25, tests/g25.py): fwd3 / adj3
at more than 32 gene blocks, fwd3c / adj3c at every hidden-chunk count 2 ... 6 and at chunk heights with and without padding
rows, under shared and per-trajectory step control and over a grid with an inner time.  The engine is held to the
reference's OWN measured distance from that truth -- its float32 runs at rtol x {0.85 ... 1.15} -- not to a float32
restatement of the algorithm:

  per case and mode   worst gradient error <= 1.5 x the largest of the reference's seven; the same for the worst dL/dy0
                      row, each row normalised by its own truth maximum
  per regime          (unit cotangents / cotangents of training scale 1/(B N)) median <= 1.25 x the reference's median

The factors are golden G12's; nothing in the bar comes from the engine.  No bar is widened for the parameter block that
the engine's controllers leave out of the adjoint norm (adjoint.py:72-78): on the CPU oracle, which implements both, the
variant without the block is within the bar at every G25 case (test_oracle_vs_golden.py prints both; at training scale
the two are identical, with unit cotangents they differ by up to 3e-6 in either direction).

Every error goes through conftest.grad_err, the cases of training scale tagged "g25-train": there the reference itself is
4e-5 ... 3.6e-4 from the truth (atol = 1e-9 dominates every adjoint tolerance and the backward solve is loosely
converged), systematically and not as jitter.  They are counted in the suite's median all the same: it stays at 4e-6.

Also asserted at every case and mode: the kernel family and its hidden chunks (HC, Hc) as planned for the device, the
trajectories against the truth, dL/dg exactly 0.0 wherever g <= 0 (as the reference's relu gives it), and that a second
identical call returns the same bits."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import g25
from conftest import ROOT, grad_err, relerr
from test_gpu_parity import TOL_DOPRI, grads_of, make_net, zero_grads

pytestmark = pytest.mark.gpu

ODEINT, ADJOINT = 2, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


@pytest.fixture(scope="module")
def gold():
    return g25.load()


@pytest.fixture(scope="module")
def fields():
    spec = importlib.util.spec_from_file_location("plan_table", os.path.join(ROOT, "tools", "plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FIELDS          # phx_debug_plan's out[]


def _solve(pa, dev, net, y0, t, G, mode):
    """one forward / backward pair: the solution [T, B, N] and the gradients as g25.stored() takes them"""
    B, N = y0.shape
    zero_grads(net)
    y = torch.from_numpy(y0).to(dev).reshape(B, 1, N).requires_grad_(True)
    tt = torch.from_numpy(np.tile(t[None], (B, 1)) if mode == "per" else t).to(dev)
    sol = pa.odeint_adjoint(net, y, tt)
    assert sol.shape == (len(t), B, 1, N)
    torch.autograd.backward(sol, torch.from_numpy(G).to(dev).reshape(len(t), B, 1, N))
    return sol.detach().cpu().numpy().reshape(len(t), B, N), dict(grads_of(net), y0=y.grad.cpu().numpy().reshape(B, N))


_SOLVED = {}


def _solved(pa, dev, shape, mode):
    """the engine at one case and mode, solved once per session: (solution, gradients, the same of a second call)"""
    if (shape, mode) not in _SOLVED:
        p, y0, t, G = g25.inputs(shape, mode)
        net = make_net(pa, dev, p)
        _SOLVED[shape, mode] = _solve(pa, dev, net, y0, t, G, mode) + _solve(pa, dev, net, y0, t, G, mode)
    return _SOLVED[shape, mode]


@pytest.mark.parametrize("shape,mode", g25.RUNS, ids=["%dx%dx%d-%s" % (s + (m,)) for s, m in g25.RUNS])
def test_g25_engine_against_the_fp64_truth(pa, dev, gold, fields, shape, mode):
    from phoenix_amd import _lib
    lib = _lib.load()
    (N, H, B), (_, family, HC, Hc) = shape, g25.CASES[g25.SHAPES.index(shape)][1:]
    p, y0, t, G = g25.inputs(shape, mode)
    assert np.allclose(g25.checksums(p), g25.checksums_of(gold, shape), rtol=1e-12, atol=0)
    # the kernels the case is there for, and their hidden chunks
    ctl = _lib.CTRL_PER_TRAJECTORY if mode == "per" else _lib.CTRL_SHARED
    kf = lib.phx_debug_forward_kernel_m(N, H, B, len(t), ctl, _lib.METHODS["dopri5"])
    ka = lib.phx_debug_adjoint_kernel_m(N, H, B, len(t), ctl, _lib.METHODS["dopri5"])
    assert (kf, ka) == (family, family)
    for op, k in ((ODEINT, kf), (ADJOINT, ka)):
        out = (C.c_longlong * len(fields))()
        assert lib.phx_debug_plan(op, k, lib.phx_device_cus(), N, H, B, len(t), ctl, _lib.METHODS["dopri5"], 1, out)
        pl = dict(zip(fields, out))
        if family == 4:
            assert (pl["HC"], pl["Hc"]) == (HC, Hc), (op, pl["HC"], pl["Hc"])
        print("plan of op %d, kernel %d at %d CUs: HC %d Hc %d hb %d TG %d TPW %d ntg %d NB %d G %d" % (
            op, k, lib.phx_device_cus(), pl["HC"], pl["Hc"], pl["hb"], pl["TG"], pl["TPW"], pl["ntg"], pl["NB"], pl["G"]))
    sol, gr, sol2, gr2 = _solved(pa, dev, shape, mode)
    truth = g25.truth_of(gold, shape, mode)
    assert relerr(sol[1:], truth["sol"]) < TOL_DOPRI
    tag = "g25-train" if g25.regime(shape) == "train" else "g25"
    e = g25.errors(g25.stored(shape, gr), truth, rel=lambda a, b: grad_err(a, b, "%s %s %s" % (tag, shape, mode)))
    print(g25.table_line("engine", shape, mode, e, gold))
    bar, bar_row, _ = g25.bars(gold, shape, mode)
    assert g25.worst(e) <= bar, (e, bar)
    assert e["row"] <= bar_row, (e["row"], bar_row)
    # the reference's relu gives a gene with g <= 0 a gradient of exactly zero; Adam makes a full step out of a 1e-12
    assert np.any(p["g"] <= 0) and np.all(gr["g"][p["g"] <= 0] == 0.0)
    assert np.array_equal(truth["g"][p["g"] <= 0], np.zeros(int(np.sum(p["g"] <= 0))))
    # a second identical call returns the same bits
    assert np.array_equal(sol, sol2)
    for k in g25.GRADS:
        assert np.array_equal(gr[k], gr2[k]), k


@pytest.mark.parametrize("regime", ["unit", "train"])
def test_g25_median_of_a_regime(pa, dev, gold, regime):
    runs = [(s, m) for s, m in g25.RUNS if g25.regime(s) == regime]
    ours = [g25.worst(g25.errors(g25.stored(s, _solved(pa, dev, s, m)[1]), g25.truth_of(gold, s, m))) for s, m in runs]
    ref = np.concatenate([g25.bars(gold, s, m)[2] for s, m in runs])
    print("%s: engine median %.2e max %.2e | reference median %.2e max %.2e" % (regime, np.median(ours), max(ours),
                                                                                np.median(ref), ref.max()))
    assert np.median(ours) <= g25.MEDIAN * np.median(ref), (np.median(ours), np.median(ref))
