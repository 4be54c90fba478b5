"""Row f4: k_hill_rhs and k_hill_simulate (csrc/phx_hill.inc) on synthetic networks of any size
(tests/test_simulator_cpu.py: synthetic_network) against float64 -- the paths the two shipped networks (350 and 690
genes: one gene per thread, increasing times, one dt_max) never take: up to HILL_GPT = 8 genes per thread with the
`gene < N` guards in the middle of a thread's list, an evaluation stack used to its last slot, NEG and unary plus,
fAct at TF <= 0, more rows than a grid's y dimension holds, decreasing times, T = 1, B = 1, spans shorter than dt_max
and spans that are rounding-sensitive multiples of it.  Run with `-m gpu`.

References: rates -- oracle.hill_oracle.rhs, Python's float64 evaluation of the expression strings (with fAct0, the
continuation fAct = 0 at TF <= 0 that the device defines; R's fAct is NaN there).  Trajectories -- a float64 restatement
of the kernel's integrator on that same rhs: classical RK4, nsub = max(1, ceil(|span| / dt_max)) equal sub-steps per
interval.  Bars: those of tests/test_simulator_cpu.py for the two entry points, 5e-6 max abs on rates and 1e-5 max-norm
relative on trajectories, the latter also per gene (no gene's max abs error over all times and samples above
1e-5 max|ref|), so that one wrong gene cannot hide among thousands of right ones.

The deep gene (a product of 24 activations, each a powf and a division) may exceed 5e-6 on a correct fp32 interpreter:
its bar is max(5e-6, 4 e32), e32 = the error of oracle.hill_oracle.interpret_programs run in float32 on the same inputs
against its float64 run, measured in the case on the CPU (the factor covers powf against numpy's pow); it never comes
from the kernel.  Measured e32 of that gene: 1.1e-7 ... 4.6e-7 in the three-row cases below (bar 5e-6) and 1.9e-6 over the 70 000 rows of
the 12-gene case (bar 7.6e-6)."""
import functools
import math
import time

import numpy as np
import pytest
import torch

from test_simulator_cpu import CHAIN, and_chain, synthetic_network, synthetic_states

pytestmark = pytest.mark.gpu

RATE_BAR, TRAJ_BAR = 5e-6, 1e-5                   # tests/test_simulator_cpu.py
PHX_ERR_BAD_ARG = 4
HILL_MAX_GENES = 8 * 1024                         # HILL_GPT * 1024 threads (csrc/phx_hill.inc)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def system(N):
    """(HillSystem on the device, float64 rhs with the strings compiled once, info) of the synthetic N-gene network;
    the rhs runs row by row on Python floats for up to 8 rows (faster there), on numpy columns above"""
    from oracle import hill_oracle
    from phoenix_amd.simulator import MAX_STACK, HillSystem
    names, exprs, info = synthetic_network(N)
    sys_ = HillSystem(names, exprs, device="cuda:0")
    assert sys_.N == N and np.array_equal(sys_.is_input, info["is_input"]) and CHAIN == MAX_STACK
    f = hill_oracle.compile_rhs(names, exprs, fact=hill_oracle.fAct0)
    return sys_, (lambda x: f(x, rowwise=np.asarray(x).size <= 8 * N)), info


def deep_gene_bar(sys_, info, x):
    """max(5e-6, 4 e32) for the rates of the deep gene at the states x (see the module docstring)"""
    from oracle import hill_oracle
    g = info["deep"]
    run = lambda dt: hill_oracle.interpret_programs(sys_.code_host, sys_.consts_host, sys_.off_host[g:g + 1],   # noqa: E731
                                                    sys_.len_host[g:g + 1], x, dtype=dt)[..., 0].astype(np.float64)
    e32 = float(np.max(np.abs(run(np.float32) - run(np.float64))))
    return max(RATE_BAR, 4 * e32), e32


def hold_rates(tag, sys_, f, info, x):
    ref = f(x)
    assert np.all(np.isfinite(ref)) and np.any(x <= 0) and np.any(x > 1)
    got = sys_.rhs(torch.from_numpy(x).to(sys_.device)).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max(axis=0)                              # per gene
    bar = np.full(sys_.N, RATE_BAR)
    bar[info["deep"]], e32 = deep_gene_bar(sys_, info, x)
    print("%s: rates max err %.2e (gene %d); deep gene err %.2e e32 %.2e bar %.1e; unary gene err %.2e"
          % (tag, err.max(), int(err.argmax()), err[info["deep"]], e32, bar[info["deep"]], err[info["unary"]]))
    assert np.all(err < bar), (tag, int(np.argmax(err / bar)), float(np.max(err / bar)))
    assert np.all(got[:, sys_.is_input] == 0)                        # exactly
    return got, ref


def nsubs(times, dt_max):
    return tuple(max(1, int(math.ceil(abs(times[i + 1] - times[i]) / dt_max))) for i in range(len(times) - 1))


def rk4_reference(f, x0, times, dt_max):
    """float64 restatement of k_hill_simulate: classical 1/6-2/6-2/6-1/6 steps, nsub equal sub-steps per interval,
    computed in float64 as the kernel computes it"""
    times = np.asarray(times, np.float64)
    y = np.asarray(x0, np.float64).copy()
    out = [y.copy()]
    for i, nsub in enumerate(nsubs(times, dt_max)):
        h = (times[i + 1] - times[i]) / nsub
        for _ in range(nsub):
            k1 = f(y)
            k2 = f(y + 0.5 * h * k1)
            k3 = f(y + 0.5 * h * k2)
            k4 = f(y + h * k3)
            y = y + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out.append(y.copy())
    return np.stack(out)


def hold_trajectories(tag, N, B, times, dt_max, want_nsub=None):
    sys_, f, info = system(N)
    if want_nsub is not None:
        assert nsubs(np.asarray(times, np.float64), dt_max) == want_nsub
    x0 = synthetic_states(N, B, info, seed=len(times))
    t0 = time.time()
    ref = rk4_reference(f, x0, times, dt_max)
    t1 = time.time()
    assert np.all(np.isfinite(ref))
    got = sys_.simulate(torch.from_numpy(x0).to(sys_.device), times, dt_max).cpu().numpy()
    assert got.shape == ref.shape == (len(times), B, N) and got.dtype == np.float32
    scale = float(np.max(np.abs(ref)))
    err = np.abs(got.astype(np.float64) - ref).max(axis=(0, 1))      # per gene, over all times and samples
    print("%s: nsub %s, trajectories max err / max|ref| %.2e (gene %d), deep gene %.2e, unary gene %.2e; max|ref| %.3f; "
          "reference %.1f s" % (tag, nsubs(times, dt_max), err.max() / scale, int(err.argmax()), err[info["deep"]] / scale,
                                err[info["unary"]] / scale, scale, t1 - t0))
    assert err.max() / scale < TRAJ_BAR                              # the max-norm bar of the shipped networks
    assert np.all(err <= TRAJ_BAR * scale), (tag, int(err.argmax()))   # ... and gene by gene
    assert np.array_equal(got[0], x0)                                # bitwise
    assert np.all(got[:, :, sys_.is_input] == x0[None][:, :, sys_.is_input])   # input genes: bitwise constant
    return got, ref


# --------------------------------------------------------------------------- rates
@pytest.mark.parametrize("N", [63, 64, 65, 1024, 1025, 2049, 8192])
def test_rhs_shapes(dev, N):
    """one wave minus / exactly / plus one gene, the block size of k_hill_rhs (256) times 4 and one more, 2049, and the
    largest network k_hill_simulate takes; states in (-0.2, 1.2)"""
    sys_, f, info = system(N)
    hold_rates("N=%d B=3" % N, sys_, f, info, synthetic_states(N, 3, info))


def test_rhs_with_more_rows_than_a_grid_dimension(dev):
    """B = 70 000 rows of a 12-gene network (`generate_dataset(derivative=True)` passes T * numsamples rows): the rows
    are strided over a capped gridDim.y, 65 535 is no limit.  Every row is compared, the first and the last included."""
    sys_, f, info = system(12)
    x = synthetic_states(12, 70000, info)
    got, ref = hold_rates("N=12 B=70000", sys_, f, info, x)
    for b in (0, 2047, 2048, 65535, 65536, 69999):
        assert np.max(np.abs(got[b] - ref[b])) < RATE_BAR and np.any(got[b] != 0)


# --------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("N,times,want", [(1025, (0.0, 0.3, 0.35, 1.05), (3, 1, 7)), (2049, (0.0, 0.3, 0.35, 1.05), (3, 1, 7)),
                                          (8192, (0.0, 0.3, 0.35), (3, 1))])
def test_simulate_with_several_genes_per_thread(dev, N, times, want):
    """1024 threads with 2 (one thread), 3 (one thread) and 8 (all threads) genes each; 0.3 / 0.1 and 0.7 / 0.1 are
    rounding-sensitive sub-step counts, taken from the restatement"""
    hold_trajectories("N=%d B=3" % N, N, 3, list(times), 0.1, want)


def test_simulate_backwards_in_time(dev):
    """decreasing times: fabs(span) sub-steps of negative h"""
    hold_trajectories("N=1025 decreasing", 1025, 3, [1.0, 0.6, 0.0], 0.1, (4, 6))


def test_simulate_a_single_time(dev):
    """T = 1: no interval, the output [1, B, N] is x0"""
    got, _ = hold_trajectories("N=1025 T=1", 1025, 3, [0.7], 0.1, ())
    assert got.shape == (1, 3, 1025)


def test_simulate_a_single_sample(dev):
    hold_trajectories("N=1025 B=1", 1025, 1, [0.0, 0.25, 0.3], 0.1, (3, 1))


def test_simulate_a_span_shorter_than_dt_max(dev):
    hold_trajectories("N=1025 span 0.004", 1025, 3, [0.0, 0.004], 0.01, (1,))


def test_simulate_with_dt_max_above_every_span(dev):
    """one RK4 step per interval, of unequal lengths"""
    hold_trajectories("N=1025 dt_max 1.0", 1025, 3, [0.0, 0.2, 0.5], 1.0, (1, 1))


# --------------------------------------------------------------------------- rejections, with nothing launched
def test_more_genes_than_a_workgroup_holds_are_rejected(dev):
    from phoenix_amd import _lib, engine
    from phoenix_amd.simulator import HillSystem
    N = HILL_MAX_GENES + 1
    names = ["G%d" % i for i in range(N)]
    sys_ = HillSystem(names, ["0.5 - G0"] + ["input gene"] * (N - 2) + ["G0 - G%d" % (N - 1)], device=dev)
    x0 = torch.rand(2, N, device=dev)
    rates = sys_.rhs(x0)                                             # k_hill_rhs has no such limit
    assert torch.equal(rates[:, N - 1], x0[:, 0] - x0[:, N - 1]) and bool((rates[:, 1:N - 1] == 0).all())
    with pytest.raises(RuntimeError, match="bad argument"):
        sys_.simulate(x0, [0.0, 0.1], 0.1)
    t64 = torch.tensor([0.0, 0.1], dtype=torch.float64, device=dev)
    out = torch.full((2, 2, N), float("nan"), device=dev)
    rc = _lib.load().phx_hill_simulate(*sys_._args(), engine._p(x0), engine._p(t64), 2, 0.1, engine._p(out), 2, N,
                                       engine._stream_ptr())
    torch.cuda.synchronize()
    assert rc == PHX_ERR_BAD_ARG and bool(torch.isnan(out).all())


def test_a_25_deep_chain_is_rejected_on_the_host(dev):
    from phoenix_amd import simulator as sim
    L = sim.MAX_STACK + 1
    names = ["R%d" % i for i in range(L)] + ["D"]
    edges = {(tf, "D"): {"from": tf, "weight": "1", "EC50": "0.3", "n": "2"} for tf in names[:L]}
    with pytest.raises(ValueError, match="deeper evaluation stack"):
        sim.HillSystem(names, ["input gene"] * L + [sim.rate_expression("D", and_chain("D", names[:L], edges), edges)], device=dev)
