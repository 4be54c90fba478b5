"""CPU-only checks of the launch planner of the persistent solve kernels (csrc/phx_plan.hpp) through phx_debug_plan: the
plans of a committed table, invariants of every plan of tools/plan_table.py's sweep, and that the workspace queries
cover the remainder launch of a batch that runs in chunks."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import GOLDEN, ROOT

LDS_BUDGET = 163840 - 1024   # csrc/phx_host.hpp
T = 2


@pytest.fixture(scope="module")
def pt():
    spec = importlib.util.spec_from_file_location("plan_table", os.path.join(ROOT, "tools", "plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from phoenix_amd import _lib
    return _lib.load()


def test_plans_equal_the_committed_table(pt, lib):
    """tests/golden/solve_plans.txt (tools/plan_table.py --cus 256 --kernels --golden): bench.py's four workloads and the
    shapes around the planners' thresholds, every kernel.  The rows were checked against the planners this one replaced;
    a planner change shows as exactly the rows it moves."""
    want = open(os.path.join(GOLDEN, "solve_plans.txt")).read().splitlines(True)
    got = list(pt.golden_lines(lib))
    shapes = {tuple(int(f[2:]) for f in w.split()[3:6]) for w in want[1:]}
    assert {(11165, 40, 256), (350, 40, 1024), (2000, 120, 23), (14691, 200, 256)} <= shapes
    assert {48, 49, 128, 129, 256} <= {s[1] for s in shapes} and {32, 33, 70000} <= {s[0] for s in shapes}
    assert {1, 16, 17, 673, 686, 4097} <= {s[2] for s in shapes}
    moved = [(w, g) for w, g in zip(want, got) if w != g]
    assert not moved and len(got) == len(want), moved[:5]


def _check(pt, cus, row):
    tag, op, k, N, H, B, ctl, m, calls, v = row
    p = dict(zip(pt.FIELDS, v))
    assert (p["N"], p["H"], p["B"], p["T"]) == (N, H, B, T), row
    assert p["TG"] * p["G"] <= cus, row
    assert p["lds"] <= LDS_BUDGET, row
    assert p["Bt"] == 16 * p["ntg"], row
    if op == pt.ODEINT and k == 4:
        assert p["Bt"] <= 64 * p["NW"], row   # k1_solve_fwd3c's controllers step one trajectory per thread
    if ctl == 0 and k != 5:
        assert p["TG"] == 1 or p["Bcall"] > 0, row   # one shared controller per batch group
    assert (p["Bcall"] > 0) == (calls > 1) and p["Bcall"] * calls == (B if calls > 1 else 0), row
    # regions: in the layout's order, 256-byte aligned, none inside another (a region the family lacks keeps offset 0)
    order = [p[f] for f in ("cnt", "part", "zbuf", "part1", "zbuf1", "scratch", "dtheta", "prof", "wimg", "hq") if f == "cnt" or p[f]]
    order.append(p["total"])
    assert all(o % 256 == 0 for o in order) and order == sorted(order), row
    assert p["cnt"] == 0 and p["part"] >= 4096 and p["zbuf"] > p["part"], row
    after_set0 = p["part1"] or p["scratch"]
    assert p["part"] + p["xbytes"] == after_set0, row   # what a fill covers ends where the next region begins
    if p["part1"]:
        assert p["zbuf1"] > p["part1"] and p["scratch"] - p["part1"] == p["xbytes"], row   # the second set is as large
    scratch_end = min(o for o in order if o > p["scratch"])
    assert p["scratch"] + p["TG"] * p["G"] * p["nvec"] * p["ntg"] * p["NB"] * 2048 <= scratch_end, row
    if op == pt.ADJOINT:
        assert p["dtheta"] + 4 * p["pp"] * p["nparts"] <= p["prof"], row   # the partials the reduce sums
    assert p["wimg"] < p["total"], row


@pytest.mark.parametrize("cus", (256, 64, 8))
def test_every_plan_of_the_sweep_keeps_the_invariants(pt, lib, cus):
    """tools/plan_table.py's grid, switches and kernels, the forward kernels also with 2, 7 and 300 calls"""
    n = 0
    for row in pt.plans(lib, cus, [(N, H, B) for N in pt.NS for H in pt.HS for B in pt.BS], pt.PLAN_ENVS, True):
        if row[9] is not None:
            _check(pt, cus, row)
            n += 1
    assert n > 10000


def _total(pt, lib, op, k, N, H, B, ctl, m, calls=1):
    v = pt.plan(lib, op, k, 256, N, H, B, ctl, m, calls)
    assert v is not None, (op, k, N, H, B, ctl, m, calls)
    return v[pt.FIELDS.index("total")]


def test_workspace_queries_cover_the_remainder_launch(pt, lib):
    """a batch that runs in chunks ends with a smaller launch, whose plan can have more batch groups or twice the gene
    tiles -- a larger layout than the chunk's: the device-free queries (sized for 256 CUs) cover both.  Not covered here:
    phx_workspace_bytes, which plans for the device's own CU count and answers for no other -- the case that once failed
    there (N = 6000, H = 200, B = 673 .. 686: k1_solve_bp does not plan H = 200, and no forward kernel takes 673 rows as one
    call) is held on the device, tests/test_plans_gpu.py."""
    shapes = [(N, H, B) for N in pt.NS for H in pt.HS for B in pt.BS]
    chunked = 0
    for N, H, B in shapes:
        # k1_solve_bp: rows per launch and launches from phx_debug_backprop_plan
        bp = (C.c_int * 8)()
        if lib.phx_debug_backprop_plan(256, N, H, B, T, 2, bp) and bp[7] > 1:
            chunk, need = bp[6], lib.phx_odeint_backprop_workspace_bytes(N, H, B, T, 0)
            assert _total(pt, lib, pt.ADJOINT, 5, N, H, chunk, 1, 2) <= need
            if B % chunk:
                chunked += 1
                assert _total(pt, lib, pt.ADJOINT, 5, N, H, B % chunk, 1, 2) <= need, (N, H, B)
            steps = 5   # ... and the checkpoint region behind it holds the chunk's rows
            assert lib.phx_odeint_backprop_workspace_bytes(N, H, B, T, steps) >= need + steps * chunk * N * 4
        # several calls with their own grids: calls per launch and kernel from phx_debug_calls_grids_plan
        for calls in pt.CALLS:
            cg = (C.c_int * 6)()
            n = lib.phx_debug_calls_grids_plan(N, H, B * calls, T, calls, 3, cg)
            if n and calls % n:
                chunked += 1
                need = lib.phx_odeint_calls_grids_workspace_bytes(N, H, B * calls, T, calls, 3)
                for launch in (n, calls % n):
                    assert _total(pt, lib, pt.ODEINT, cg[0], N, H, B * launch, 0, 3, launch) <= need, (N, H, B, calls, launch)
    assert chunked > 100
