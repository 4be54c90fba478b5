"""k1_solve_bp (the backward pass of `odeint(method="euler" | "midpoint" | "rk4")`) at every kind of launch geometry its
planner gives on the 256 CUs of an MI355X, against the float64 torch arbiter of tests/test_backprop_gpu.py (a plain torch
restatement of ODENet.forward stepped by phoenix_amd.generic.integrate and differentiated by autograd).  Run with `-m gpu`.

Every case first asserts, through phx_debug_backprop_plan, the geometry it is there for (tests/test_backprop_cpu.py holds
the same table to the planner without a device), then compares the solution, dL/dy0 and the six parameter gradients.  The
bar of a quantity is max(TOL_FIXED, 2 e32), e32 = the error of the same arbiter run in float32 against its float64 run,
measured in the case: it comes from the reference, never from the kernel.

nb_ht8: N = 350, H = 100 keeps two gene blocks of the eight-tile kernel in LDS, and B = 1530 is the smallest multiple of
64 minus 6 for which the planner asks for them (B = 1466 still gives every gene block a workgroup of its own)."""

import numpy as np
import pytest
import torch

from test_backprop_cpu import GEOMETRY, bp_plan
from test_backprop_gpu import KEYS, TOL_FIXED, arbiter, errors, make_net, rand_params, run_odeint

pytestmark = pytest.mark.gpu

T5 = (0.0, 2.0, 3.0, 7.0, 9.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def device_plan(name):
    """the plan of GEOMETRY[name] on THIS device, asserted to be the geometry the case is there for"""
    from phoenix_amd import _lib
    cus = _lib.load().phx_device_cus()
    assert cus == 256, "the geometry table is that of an MI355X (256 CUs); this device reports %d" % cus
    (N, H, B), want = GEOMETRY[name]
    got = bp_plan(N, H, B, cus=0)
    assert got is not None, name
    print("%s N=%d H=%d B=%d plan %s" % (name, N, H, B, got))
    assert {k: got[k] for k in want} == want, (name, got)
    return got


def inputs(N, H, B, seed, t):
    """parameters, start states and cotangents as tests/test_backprop_gpu.py check_against_arbiter draws them"""
    p = rand_params(N, H, seed=seed, std=0.05)
    r = np.random.RandomState(seed + 1)
    y0 = np.clip(r.beta(2, 2, size=(B, N)) + r.uniform(-0.25, 0.25, size=(1, N)), 0, 1).astype(np.float32)
    G = (r.randn(len(t), B, N) / (B * N)).astype(np.float32)
    return p, y0, G


def hold(tag, got, ref64, ref32):
    e32 = errors(ref32, ref64)
    errs = errors(got, ref64)
    for k in errs:
        print("%s %-8s err=%.2e e32=%.2e" % (tag, k, errs[k], e32[k]))
    print("%s worst err/bar %.3f" % (tag, max(errs[k] / max(TOL_FIXED, 2 * e32[k]) for k in errs)))
    for k in errs:
        assert errs[k] < max(TOL_FIXED, 2 * e32[k]), (tag, k, errs[k], e32[k])


def check(pa, dev, name, seed, method, h, t=T5):
    (N, H, B), _ = GEOMETRY[name]
    t = np.array(t, np.float32)
    p, y0, G = inputs(N, H, B, seed, t)
    ref64 = arbiter(pa, p, dev, torch.float64, y0, t, G, method, h)
    ref32 = arbiter(pa, p, dev, torch.float32, y0, t, G, method, h)
    net = make_net(pa, dev, p)
    got = run_odeint(pa, net, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(G).to(dev), method, h)
    hold("%s/%s/h=%s" % (name, method, h), got, ref64, ref32)


ALL3 = ("euler", "midpoint", "rk4")


# ------------------------------------------------------------------------------------------ 1: one workgroup per tile
@pytest.mark.parametrize("h", [None, 0.75])
@pytest.mark.parametrize("method", ALL3)
def test_g1_one_workgroup_owns_every_exchange_row(pa, dev, method, h):
    """G = 1: the owner stride of reduce_owned is 1 and there is no other member to wait for"""
    d = device_plan("g1")
    assert d["G"] == 1 and d["TG"] * d["ntg"] == 1
    check(pa, dev, "g1", 31, method, h)


# ------------------------------------------------------------------------------------------ 2: more than 16 members
@pytest.mark.parametrize("method, h", [("rk4", None), ("rk4", 0.75), ("euler", None)])
def test_g17_second_chunk_of_members_holds_one(pa, dev, method, h):
    """G = 17: reduce_owned waits for 16 members, then for 1; the last gene block holds 18 genes"""
    d = device_plan("g17")
    assert d["G"] == 17 and GEOMETRY["g17"][0][0] - 32 * (d["nblk"] - 1) == 18
    check(pa, dev, "g17", 33, method, h)


@pytest.mark.parametrize("h", [None, 0.75])
def test_dec_decreasing_time_at_g17(pa, dev, h):
    device_plan("g17")
    check(pa, dev, "g17", 35, "rk4", h, t=T5[::-1])


@pytest.mark.parametrize("method, h", [("rk4", None), ("rk4", 0.75), ("midpoint", 0.75)])
def test_g35_three_chunks_of_members_two_tiles(pa, dev, method, h):
    """G = 35 = 16 + 16 + 3 members, two trajectory tiles (the second holds 4 rows)"""
    d = device_plan("g35")
    assert d["G"] == 35 and d["ntg"] == 2
    check(pa, dev, "g35", 37, method, h)


# ------------------------------------------------------------------------------------------ 3: several gene blocks in LDS
@pytest.mark.parametrize("method, h", [("rk4", None), ("rk4", 0.75), ("euler", None), ("midpoint", None)])
def test_nb2_ragged_last_workgroup(pa, dev, method, h):
    """NB = 2 over 11 gene blocks: the last workgroup of a group holds one block (nbl = 1); the last tile holds 10 rows"""
    d = device_plan("nb2")
    N, H, B = GEOMETRY["nb2"][0]
    assert d["NB"] == 2 and d["nblk"] - (d["G"] - 1) * d["NB"] == 1 and B - 16 * (-(-B // 16) - 1) == 10
    check(pa, dev, "nb2", 39, method, h)


def test_nbmax_most_gene_blocks_per_workgroup(pa, dev):
    """NB = 8, the planner's cap, G = 4.  LDS holds eight gene blocks up to H = 34; at H = 40 it holds seven, and the
    planner serves N = 1000, B = 4096 in two launches of 2048 rows with NB = 4, G = 8 (the next test)."""
    d = device_plan("nbmax")
    assert d["HT"] == 3 and d["NB"] >= 6
    check(pa, dev, "nbmax", 41, "rk4", None)


def test_nb4_in_two_equal_launches(pa, dev):
    d = device_plan("nb4x2")
    assert d["NB"] == 4 and d["launches"] == 2
    check(pa, dev, "nb4x2", 42, "rk4", None)


@pytest.mark.parametrize("method, h", [("rk4", None), ("rk4", 0.75), ("euler", 0.75)])
def test_nb_ht8_two_gene_blocks_of_the_eight_tile_kernel(pa, dev, method, h):
    """HT = 8 with NB = 2 (nbl = 1 in the last workgroup), last tile 10 rows"""
    d = device_plan("nb_ht8")
    assert d["HT"] == 8 and d["NB"] >= 2 and GEOMETRY["nb_ht8"][0][2] % 16 != 0
    check(pa, dev, "nb_ht8", 43, method, h)


# ------------------------------------------------------------------------------------------ 4: padding waves
@pytest.mark.parametrize("h", [None, 0.3])
@pytest.mark.parametrize("method", ALL3)
def test_pad_last_group_with_one_real_tile(pa, dev, method, h):
    """TG = 2 x ntg = 4: the second group has one tile with 6 real rows and three waves that run padding trajectories only"""
    d = device_plan("pad")
    B = GEOMETRY["pad"][0][2]
    assert d["TG"] == 2 and d["ntg"] == 4 and d["HT"] == 8 and B - 64 == 6
    check(pa, dev, "pad", 45, method, h)


# ------------------------------------------------------------------------------------------ 5: per-sample grids
def grid_steps(t0, t1, h):
    """grid steps of one row under a step size, formed in float32 as the grid is (generic._step_grid)"""
    a, b = (np.float32(t0), np.float32(t1)) if t1 > t0 else (np.float32(-t0), np.float32(-t1))
    return max(int(np.ceil((b - a) / np.float32(h) + np.float32(1))), 2) - 1


@pytest.mark.parametrize("h", [0.5, None])
def test_per_sample_grids_at_pad(pa, dev, h):
    """t [B, 2] at the `pad` geometry: one grid per row, both directions inside a tile and, with a step size, other step
    counts in every tile (nmax by shuffle, dt = 0 past a row's own grid).  Cotangent on the end state only.  Reference:
    the arbiter called once per row, parameter gradients summed over the rows."""
    device_plan("pad")
    N, H, B = GEOMETRY["pad"][0]
    p, y0, G = inputs(N, H, B, 47, (0, 1))
    G[0] = 0
    r = np.random.RandomState(48)
    t = np.stack([np.zeros(B), r.uniform(1, 9, B)], 1).astype(np.float32)
    dec = r.rand(B) < 0.25
    t[dec] = np.stack([np.full(B, 9.0), r.uniform(0, 8, B)], 1).astype(np.float32)[dec]
    assert all(0 < dec[i:i + 16].sum() < 16 for i in range(0, 64, 16)), "every full tile must mix both directions"
    if h is not None:
        n = np.array([grid_steps(t[b, 0], t[b, 1], h) for b in range(B)])
        print("grid steps per row:", n.tolist())
        assert all(len(set(n[i:i + 16])) > 1 for i in range(0, B, 16)), "every tile must mix step counts"

    def per_row(dtype):
        rows = [arbiter(pa, p, dev, dtype, y0[b:b + 1], t[b], G[:, b:b + 1], "rk4", h) for b in range(B)]
        out = {"sol": np.concatenate([x["sol"][1] for x in rows]), "grad_y0": np.concatenate([x["grad_y0"] for x in rows])}
        out.update({"grad_" + k: sum(x["grad_" + k] for x in rows) for k in KEYS})
        return out

    ref64, ref32 = per_row(torch.float64), per_row(torch.float32)
    net = make_net(pa, dev, p)
    got = run_odeint(pa, net, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(G).to(dev), "rk4", h)
    got["sol"] = got["sol"][1]
    hold("ps/pad/h=%s" % h, got, ref64, ref32)


# ------------------------------------------------------------------------------------------ 6: the chunk driver
@pytest.mark.parametrize("h", [None, 0.75])
def test_chunked_batch_with_a_small_second_launch(pa, dev, h):
    """4096 + 40 rows at N = 700: two launches whose plans differ (NB = 6, TG = 64, then NB = 1, TG = 1: the workspace is
    laid out anew for the second, bp_base_bytes sizes it for the larger of the two), against the arbiter on the whole batch"""
    first = device_plan("chunk")
    N, H, B = GEOMETRY["chunk"][0]
    assert first["launches"] == 2 and first["chunk_rows"] == 4096
    second = device_plan("chunk_tail")
    assert GEOMETRY["chunk_tail"][0] == (N, H, B - first["chunk_rows"])
    assert (second["NB"], second["TG"]) != (first["NB"], first["TG"]), (first, second)
    check(pa, dev, "chunk", 49, "rk4", h)


@pytest.mark.parametrize("h", [None, 0.75])
def test_b4136_one_launch_of_65_groups(pa, dev, h):
    """N = 350, 4096 + 40 rows: the planner keeps this batch in ONE launch (TG = 65, NB = 4, G = 3, last workgroup
    nbl = 3); the last group holds 40 rows: two full tiles, one of 8 rows and a padding wave"""
    d = device_plan("b4136")
    assert d["launches"] == 1 and d["TG"] == 65 and d["nblk"] - (d["G"] - 1) * d["NB"] == 3
    check(pa, dev, "b4136", 51, "rk4", h)
