"""The kernels that serve `odeint_adjoint(method="euler" | "midpoint" | "rk4")` -- k1_solve_fwd forward, k1_solve_adj2 /
k1_solve_adj backward, and the VALU kernels k_solve_fwd / k_solve_adj where none plans the batch -- at every kind of launch geometry
their planners give on the 256 CUs of an MI355X, against the float64 truth of tests/g26.py.  Run with `-m gpu`.

Every case first asserts the kernels the device dispatches (phx_debug_forward_kernel_m / phx_debug_adjoint_kernel_m, with
the stepped flag 0x100 under a step size) and, through phx_debug_plan on the device's own CU count, the geometry it is
there for (tests/test_fixed_grid_cpu.py holds the same table to the planner without a device), prints both, runs
`odeint_adjoint` through the public entry point and holds the solution, dL/dy0 and the six parameter gradients to the
truth: globally, by trajectory row and by block of 32 genes (g26.figures), each under max(TOL_FIXED, 2 e32) with e32 the
float32 references' own figure, measured in the case on the device.  The condition that keeps that bar at TOL_FIXED is
asserted on the CPU, in tests/test_fixed_grid_cpu.py."""
import numpy as np
import pytest
import torch

import g26
from test_backprop_gpu import grads_of, make_net, zero_grads
from test_fixed_grid_cpu import (ADJOINT, CHUNKED, CHUNKS, EDGE_ROWS, EDGES, GEOMETRY, ODEINT, PER_SAMPLE, SEEDS, T, T5,
                                 check_row, control_of, per_sample_grid, references, runs_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def set_env(monkeypatch, name):
    import plan_table as pt
    for k in pt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in GEOMETRY[name][0][4].items():
        monkeypatch.setenv(k, v)


def device_dispatch(name, method, fwd_step, bwd_step):
    """the kernels and plans of GEOMETRY[name] on THIS device, asserted to be the ones the case is there for"""
    from phoenix_amd import _lib
    lib = _lib.load()
    cus = lib.phx_device_cus()
    assert cus == 256, "the geometry table is that of an MI355X (256 CUs); this device reports %d" % cus
    (N, H, B, control, env), fwd, bwd = GEOMETRY[name]
    assert control == "per_trajectory" or not (fwd_step or bwd_step), "a step size plans per trajectory: not this row's geometry"
    m = _lib.METHODS[method]
    kf = lib.phx_debug_forward_kernel_m(N, H, B, T, control_of(control), m | (0x100 if fwd_step else 0))
    ka = lib.phx_debug_adjoint_kernel_m(N, H, B, T, control_of(control), m | (0x100 if bwd_step else 0))
    print("%s: forward kernel %d, backward kernel %d (0: the VALU kernel of the direction)" % (name, kf, ka))
    assert kf == (fwd["kernel"] if fwd else 0) and ka == (bwd["kernel"] if bwd else 0), (name, kf, ka)
    check_row(name, cus=cus)


def run_adjoint(pa, net, dev, y0, t, G, method, h, ah, control):
    """solution and the seven gradients of sum(G * odeint_adjoint(...)) through the public entry point"""
    zero_grads(net)
    y0r = torch.from_numpy(y0).to(dev).requires_grad_(True)
    options = {}
    if control == "per_trajectory" and t.ndim == 1:
        options["batch_control"] = "per_trajectory"
    if h:
        options["step_size"] = h
    sol = pa.odeint_adjoint(net, y0r, torch.from_numpy(t).to(dev), method=method, options=options or None,
                            adjoint_options={"step_size": ah} if ah else None)
    (sol * torch.from_numpy(G).to(dev)).sum().backward()
    out = {"sol": sol.detach().cpu().numpy(), "grad_y0": y0r.grad.cpu().numpy()}
    out.update({"grad_" + k: v for k, v in grads_of(net).items()})
    return out


def check(pa, dev, oracle, monkeypatch, name, method, h, t=None, ah=None, seed=0, arbiter_dev=None):
    set_env(monkeypatch, name)
    device_dispatch(name, method, h, ah or h)
    (p, y0, t, G), truth, e32 = references(name, method, h, t=t, ah=ah, dev=arbiter_dev or dev, orc=oracle, seed=seed)
    got = run_adjoint(pa, make_net(pa, dev, p), dev, y0, t, G, method, h, ah, GEOMETRY[name][0][3])
    tag = "%s/%s/h=%s" % (name, method, h) + ("/ah=%s" % ah if ah else "")
    print("%s e32 worst %.2e" % (tag, max(e32.values())))
    g26.hold(tag, got, truth, e32)
    return (p, y0, t, G), truth, e32, got


# ------------------------------------------------------------------------------------------ 1: every row of the table
@pytest.mark.parametrize("name, method, h", [(n, m, h) for n in sorted(GEOMETRY) if n not in PER_SAMPLE for m, h in runs_of(n)])
def test_every_geometry_against_the_truth(pa, dev, oracle, monkeypatch, name, method, h):
    check(pa, dev, oracle, monkeypatch, name, method, h)


# ------------------------------------------------------------------------------------------ 2: the time axis
@pytest.mark.parametrize("name", EDGE_ROWS)
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_time_axis_edges(pa, dev, oracle, monkeypatch, edge, name):
    """a decreasing grid, a backward step of its own, output times ON step-grid points, a step longer than every interval,
    a float64 grid none of whose values is a float32 -- on one small shape per backward kernel form (T5 under
    g26.STEP already has a short last sub-step in the intervals of length 1 and 2 and a step longer than the interval of
    length 0.5: every per_trajectory case of test 1)"""
    t, h, ah = EDGES[edge]
    check(pa, dev, oracle, monkeypatch, name, "rk4", h, t=t, ah=ah, seed=1)


@pytest.mark.parametrize("h", [None, 0.3])
@pytest.mark.parametrize("name", PER_SAMPLE)
def test_per_sample_grids(pa, dev, oracle, monkeypatch, name, h):
    """t [B, 5]: another interval length in every row, both directions inside a tile; with a step size the rows of a tile
    take different numbers of sub-steps.  The arbiter solves the rows one by one (on the CPU: 2 B small solves)."""
    B = GEOMETRY[name][0][2]
    check(pa, dev, oracle, monkeypatch, name, "rk4", h, t=per_sample_grid(B, SEEDS[name]), seed=2, arbiter_dev="cpu")


# ------------------------------------------------------------------------------------------ 3: the chunk driver
@pytest.mark.parametrize("h", [None, g26.STEP])
def test_chunked_batch(pa, dev, h):
    """N = 7000, H = 226, 557 rows per trajectory: the forward solve runs in launches of 512 + 45 rows, the backward solve
    in 256 + 256 + 45, whose parameter gradients add up in the caller's arrays.  Held to the truth of the WHOLE batch --
    every row on both sides of every launch boundary, and the summed parameter gradients by gene block."""
    from phoenix_amd import _lib
    lib = _lib.load()
    assert lib.phx_device_cus() == 256
    N, H, B = CHUNKED
    per = _lib.CTRL_PER_TRAJECTORY
    m = _lib.METHODS["rk4"] | (0x100 if h else 0)
    assert lib.phx_debug_forward_kernel_m(N, H, B, T, per, m) == 1 and lib.phx_debug_adjoint_kernel_m(N, H, B, T, per, m) == 1
    launches = [lib.phx_debug_solve_launches(op, N, H, B, T, per, _lib.METHODS["rk4"]) for op in (ODEINT, ADJOINT)]
    print("chunked N=%d H=%d B=%d: launches forward %d backward %d, rows per launch %d / %d" % (
        N, H, B, launches[0], launches[1], CHUNKS[ODEINT][0], CHUNKS[ADJOINT][0]))
    assert launches == [-(-B // CHUNKS[ODEINT][0]), -(-B // CHUNKS[ADJOINT][0])] == [2, 3]
    (p, y0, t, G), truth, e32 = references("chunked", "rk4", h, dev=dev)
    got = run_adjoint(pa, make_net(pa, dev, p), dev, y0, t, G, "rk4", h, None, "per_trajectory")
    print("chunked/h=%s e32 worst %.2e" % (h, max(e32.values())))
    g26.hold("chunked/rk4/h=%s" % h, got, truth, e32)


# ------------------------------------------------------------------------------------------ 4: cheap properties
@pytest.mark.parametrize("name", ["h7_b100_p", "n1100_b61_p"])
@pytest.mark.parametrize("h", [None, g26.STEP])
def test_rerun_is_bit_identical_and_rows_stand_alone(pa, dev, oracle, monkeypatch, name, h):
    """a second run on the kept workspace gives the same bits; rows of the batch solved alone (another geometry, another
    summation order over the groups: not bitwise) equal the batch's rows within the bar, and the truth's"""
    (p, y0, t, G), truth, e32, got = check(pa, dev, oracle, monkeypatch, name, "rk4", h)
    net = make_net(pa, dev, p)
    control = GEOMETRY[name][0][3]
    again = run_adjoint(pa, net, dev, y0, t, G, "rk4", h, None, control)
    for k in g26.QUANT:
        assert np.array_equal(got[k], again[k]), k
    rows = np.r_[0:5, len(y0) - 2:len(y0)]
    alone = run_adjoint(pa, net, dev, y0[rows], t, np.ascontiguousarray(G[:, rows]), "rk4", h, None, control)
    for k, ax, baxis in (("sol", (0, 2), 1), ("grad_y0", (1,), 0)):      # (axes of one row's entries, the batch axis)
        part, whole = alone[k].astype(np.float64), np.take(got[k], rows, axis=baxis).astype(np.float64)
        want = np.take(truth[k], rows, axis=baxis)
        e = {"alone vs batch": g26._worst(part, whole, ax), "alone vs truth": g26._worst(part, want, ax)}
        print("%s/h=%s %s by row: %s (bar %.1e)" % (name, h, k, e, g26.bar(e32, "row:" + k)))
        assert all(v < g26.bar(e32, "row:" + k) for v in e.values()), (k, e)
