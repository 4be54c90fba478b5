"""CPU-only checks of the Hill simulator's pair knockouts (phx_hill_knockout_sets, include/phoenix_hip.h;
`HillSystem.knockouts` with held sets, `HillSystem.coregulator_pairs` / `knockout_pairs`, `epistasis_recovery`): the symbol
exists, every refusal answers before a device call -- and `knockouts_reference` with sets, which
tests/test_hillko_pairs_gpu.py holds the kernel to, is itself held to the "input gene" form of a held set, to a case worked
by hand and to the symmetries of a set; `coregulator_pairs` against the expression text; `epistasis_recovery_scores` on
planted arrays."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols
from test_hillko_cpu import DT_MAX, TIMES, cpu_system, descendants
from test_knockout_pairs_cpu import reference64_pairs
from test_simulator_cpu import synthetic_network, synthetic_states

BAD_ARG = 4
PAIR = (1, 39)      # two genes of synthetic_network(65) that meet in a gate: the pair the GPU screen is not vacuous on


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


# --------------------------------------------------------------------------- the C ABI
def test_new_symbol_is_exported_and_declared():
    mod, lib = _lib()
    name = "phx_hill_knockout_sets"
    assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name)
    assert lib.phx_abi_version() == 7       # an additive change
    from phoenix_amd import simulator
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phoenix_hip.h")).read()
    assert "#define PHX_HILL_HOLD_MAX %d" % simulator.HOLD_MAX in src


def _call(lib, code=0x1000, off=0x2000, len_=0x3000, consts=0x4000, x0=0x5000, times=0x6000, T=4, dt_max=0.1,
          genes=((0, 3), (-1, -1), (7, -1)), values=((0.0, 0.5), (0.0, 0.0), (1.7, 0.0)), width=None, K=None, out=0x7000, B=3,
          N=8):
    """phx_hill_knockout_sets with made-up device addresses: only calls that must return before touching the device"""
    flat_g = None if genes is None else [g for row in genes for g in row]
    flat_v = None if values is None else [v for row in values for v in row]
    g = None if flat_g is None else (C.c_int * len(flat_g))(*flat_g)
    v = None if flat_v is None else (C.c_float * len(flat_v))(*flat_v)
    width = (len(genes[0]) if genes is not None else 2) if width is None else width
    K = (len(genes) if genes is not None else 3) if K is None else K
    return lib.phx_hill_knockout_sets(code, off, len_, consts, x0, times, T, dt_max, g, v, width, K, out, B, N, None)


def test_refusals_with_nothing_launched():
    _, lib = _lib()
    for name in ("code", "off", "len_", "consts", "x0", "times", "genes", "values", "out"):      # null lists among them
        assert _call(lib, **{name: None}) == BAD_ARG, name
    for name in ("B", "N", "K", "T"):
        assert _call(lib, **{name: 0}) == BAD_ARG and _call(lib, **{name: -1}) == BAD_ARG, name
    for dt in (0.0, -0.1, float("nan")):
        assert _call(lib, dt_max=dt) == BAD_ARG, dt
    assert _call(lib, N=8193, genes=((0, 8192),), values=((0.0, 0.0),)) == BAD_ARG
    # the width: 1 .. PHX_HILL_HOLD_MAX (the lists are long enough for the rows a wrong width would read)
    wide = dict(genes=((0, 1, 2, 3, 4), (5, 6, 7, -1, -1), (-1,) * 5), values=((0.0,) * 5,) * 3)
    assert _call(lib, width=5, **wide) == BAD_ARG and _call(lib, width=0, **wide) == BAD_ARG
    assert _call(lib, width=-1, **wide) == BAD_ARG
    # a gene twice in a row, next to each other and apart, at the same level or not
    assert _call(lib, genes=((0, 3), (5, 5), (7, -1))) == BAD_ARG
    assert _call(lib, genes=((0, 1, 2, 0),), values=((0.0, 0.0, 0.0, 1.0),)) == BAD_ARG
    assert _call(lib, genes=((0, -1, 0),), values=((0.5, 0.0, 0.5),)) == BAD_ARG
    # entries outside -1 .. N - 1 (N = 8)
    assert _call(lib, genes=((0, 3), (-1, -2), (7, -1))) == BAD_ARG
    assert _call(lib, genes=((0, 3), (-1, -1), (7, 8))) == BAD_ARG
    assert _call(lib, genes=((-2,),), values=((0.0,),)) == BAD_ARG and _call(lib, genes=((8,),), values=((0.0,),)) == BAD_ARG
    # a level that is not finite on a live entry, in either column
    for bad in (float("inf"), -float("inf"), float("nan")):
        assert _call(lib, values=((0.0, bad), (0.0, 0.0), (1.7, 0.0))) == BAD_ARG, bad
        assert _call(lib, values=((0.0, 0.5), (0.0, 0.0), (bad, 0.0))) == BAD_ARG, bad
    # K * B beyond int
    assert _call(lib, B=(1 << 31) // 3 + 1) == BAD_ARG
    assert _call(lib, genes=((0, 1), (2, 3)), values=((0.0, 0.0),) * 2, B=1 << 30) == BAD_ARG


def test_a_nan_level_on_a_pad_passes_the_argument_checks():
    """The level of a -1 entry is not looked at.  A call that passes the checks goes on to launch, so with made-up addresses
    it can be made only where no device would take the launch: there it answers PHX_ERR_LAUNCH, not PHX_ERR_BAD_ARG.  Where
    there is a device, tests/test_hillko_pairs_gpu.py makes the same call on real buffers."""
    mod, lib = _lib()
    nan = float("nan")
    from phoenix_amd.simulator import _knockout_set_args
    assert _knockout_set_args("knockouts", 8, [(0, -1), -1, (-1, 7)], [(0.5, nan), nan, (nan, 1.7)]) == \
        ([(0,), (), (7,)], [(0.5,), (), (1.7,)])
    if not torch.cuda.is_available():      # made-up addresses must not reach a device
        rc = _call(lib, values=((0.0, 0.5), (nan, nan), (1.7, nan)))
        assert rc != BAD_ARG and rc != 0, rc
    assert _call(lib, values=((0.0, 0.5), (nan, nan), (nan, 0.0))) == BAD_ARG      # ... on the live entry of the same row


# --------------------------------------------------------------------------- knockouts_reference with sets
def _as_inputs(names, exprs, held):
    from phoenix_amd.simulator import HillSystem
    return HillSystem(names, [e if i not in held else "input gene" for i, e in enumerate(exprs)], device="cpu")


def test_a_held_set_is_a_set_of_input_genes_bit_for_bit():
    from phoenix_amd.simulator import knockouts_reference
    names, exprs, info = synthetic_network(65)
    sys_, _ = cpu_system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    free = knockouts_reference(sys_, x0, TIMES, [-1], [0.0], DT_MAX)[:, 0]
    for held, levels in ((PAIR, (0.0, 0.0)), ((info["deep"], 7, 64, 1), (0.3, -0.15, 1.7, 0.0))):
        got = knockouts_reference(sys_, x0, TIMES, [held], [levels], DT_MAX)[:, 0]
        x1 = x0.astype(np.float64)
        x1[:, list(held)] = levels
        want = knockouts_reference(_as_inputs(names, exprs, held), x1, TIMES, [-1], [0.0], DT_MAX)[:, 0]
        assert got.dtype == np.float64 and np.array_equal(got, want) and not np.array_equal(got, free)
        for g, v in zip(held, levels):
            assert np.all(got[:, :, g] == v)
        # one level for the whole set
        same = knockouts_reference(sys_, x0, TIMES, [held], [0.25], DT_MAX)[:, 0]
        assert np.array_equal(same, knockouts_reference(sys_, x0, TIMES, [held], [(0.25,) * len(held)], DT_MAX)[:, 0])


def test_the_symmetries_of_a_set():
    from phoenix_amd.simulator import knockouts_reference
    sys_, info = cpu_system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    a, b = PAIR
    genes = [(a,), a, (a, b), (b, a), (), -1, (a, -1, b), [b, a]]
    values = [1.7, 1.7, (0.4, -0.1), (-0.1, 0.4), 9.0, 0.0, (0.4, float("nan"), -0.1), np.array([-0.1, 0.4])]
    ref = knockouts_reference(sys_, x0, TIMES, genes, values, DT_MAX)
    assert ref.shape == (len(TIMES), 8, 3, 65)
    assert np.array_equal(ref[:, 0], ref[:, 1])                       # a 1-tuple is the int entry
    assert np.array_equal(ref[:, 1], knockouts_reference(sys_, x0, TIMES, [a], [1.7], DT_MAX)[:, 0])      # ... of the plain list
    assert np.array_equal(ref[:, 2], ref[:, 3])                       # (a, b) is (b, a)
    assert np.array_equal(ref[:, 4], ref[:, 5]) and np.array_equal(ref[0, 4], x0.astype(np.float64))      # () is -1
    assert np.array_equal(ref[:, 6], ref[:, 2]) and np.array_equal(ref[:, 7], ref[:, 2])      # padding, lists and arrays
    assert not np.array_equal(ref[:, 2], ref[:, 1]) and not np.array_equal(ref[:, 2], ref[:, 5])
    ref32 = knockouts_reference(sys_, x0, TIMES, genes[:4], values[:4], DT_MAX, dtype=np.float32)
    assert ref32.dtype == np.float32 and np.array_equal(ref32[:, 2], ref32[:, 3]) and np.abs(ref32 - ref[:, :4]).max() < 1e-4


def test_pair_knockouts_on_a_case_worked_by_hand():
    """A, B inputs, C' = A B - C (an AND gate), D' = A + B - D (additive).  Unheld, C = ab + (c0 - ab) e^-t; with A or B or
    both at 0, C = c0 e^-t: the interaction d_ab - (d_a + d_b) on C is ab (1 - e^-t).  On D every knockout subtracts its own
    term, a (1 - e^-t) or b (1 - e^-t): the interaction is 0.  Bar 1e-9: RK4's global error on y' = c - y is at most
    |y0 - c| t h^4 / 120, about 1e-10 at h = 0.01, t <= 1.3, |y0 - c| <= 2, and an interaction combines four solves."""
    from phoenix_amd.simulator import HillSystem, knockouts_reference
    sys_ = HillSystem(["A", "B", "C", "D"], ["input gene", "input gene", "A * B - C", "A + B - D"], device="cpu")
    assert sys_.coregulator_pairs() == [(0, 1)]
    x0 = np.array([[0.9, 0.7, 0.2, 1.5], [0.4, 1.2, 1.4, 0.1]])
    times = np.array([0.0, 0.5, 1.3])
    out = knockouts_reference(sys_, x0, times, [-1, 0, 1, (0, 1)], 0.0, 0.01)
    base, da, db, dab = out[:, 0], out[:, 1] - out[:, 0], out[:, 2] - out[:, 0], out[:, 3] - out[:, 0]
    e = dab - (da + db)
    grow = (1.0 - np.exp(-times))[:, None]
    a0, b0 = x0[None, :, 0], x0[None, :, 1]
    assert np.max(np.abs(base[:, :, 2] - (a0 * b0 + (x0[None, :, 2] - a0 * b0) * (1 - grow)))) < 1e-9
    assert np.max(np.abs(e[:, :, 2] - a0 * b0 * grow)) < 1e-9
    assert np.max(np.abs(e[:, :, 3])) < 1e-9 and np.max(np.abs(dab[:, :, 3] + (a0 + b0) * grow)) < 1e-9
    assert np.all(out[:, 3, :, :2] == 0) and np.all(e[0] == 0)
    # the float64 scoring formulas the GPU screen is held to, on these trajectories
    K, G, T, B = 1, 2, len(times), 2
    sc, isc, sh, mg, it, im = reference64_pairs(base, out[:, 1:3].reshape(T, G * B, 4), out[:, 3], [0], [1], [0, 1])
    want_c = np.mean(a0 * b0 * grow[1:])
    assert abs(it[0, 2] - want_c) < 1e-9 and abs(it[0, 3]) < 1e-9 and abs(isc[0] - want_c / 2) < 1e-9


def test_the_interaction_is_exactly_zero_off_the_common_descendants():
    """what the issue's CPU probe found at N = 65: holding genes 1 and 39 at 0 gives a mean interaction of 0.163 max|ref| on
    a common descendant, and exactly 0 -- in float64 numpy -- at every gene that is not a common descendant of both"""
    from phoenix_amd.simulator import knockouts_reference
    sys_, info = cpu_system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    a, b = PAIR
    ref = knockouts_reference(sys_, x0, TIMES, [-1, a, b, (a, b)], 0.0, DT_MAX)
    scale = float(np.max(np.abs(ref)))
    e = (ref[1:, 3] - ref[1:, 0]) - ((ref[1:, 1] - ref[1:, 0]) + (ref[1:, 2] - ref[1:, 0]))
    common = descendants(sys_, a) & descendants(sys_, b)
    zero = ~common
    zero[[a, b]] = False      # the held genes are no targets: where b is downstream of a, d_ab = d_b there and e = -d_a
    common[[a, b]] = False
    assert common.any() and zero.any() and np.all(e[:, :, zero] == 0)
    mean = np.abs(e.mean(axis=(0, 1)))
    print("pair %r: %d common descendants, largest |mean interaction| %.3f of max|ref|" % (PAIR, common.sum(), mean.max() / scale))
    assert mean.max() > 0.1 * scale


# --------------------------------------------------------------------------- coregulator_pairs
def test_coregulator_pairs_against_the_expression_text():
    names, exprs, info = synthetic_network(65)
    sys_, _ = cpu_system(65)
    index = {n: i for i, n in enumerate(names)}
    want = set()
    for j, expr in enumerate(exprs):
        read = sorted(set(index[w] for w in re.findall(r"[A-Za-z_]\w*", expr) if w in index) - {j})
        want.update(itertools.combinations(read, 2))
    got = sys_.coregulator_pairs()
    assert got == sorted(want) and PAIR in got and all(a < b for a, b in got) and len(got) > 65
    some = sorted(set(g for p in got[:40:3] for g in p))
    sub = sys_.coregulator_pairs(genes=some)
    assert sub == [p for p in got if p[0] in some and p[1] in some] and 0 < len(sub) < len(got)
    assert sys_.coregulator_pairs(genes=np.array(some)) == sub and sys_.coregulator_pairs(genes=[PAIR[0]]) == []
    with pytest.raises(ValueError, match="coregulator_pairs"):
        sys_.coregulator_pairs(genes=[0, 65])
    with pytest.raises(TypeError, match="coregulator_pairs"):
        sys_.coregulator_pairs(genes=[0.5])


# --------------------------------------------------------------------------- recovery statistics
def test_epistasis_recovery_scores_on_planted_arrays():
    import phoenix_amd
    from phoenix_amd.analysis import recovery_scores
    pairs = [(1, 3), (0, 2), (4, 0)]
    true = np.array([[1.0, 9.0, -2.0, 7.0, 0.05, 0.0],      # (1, 3): columns 1 and 3 are left out, column 5 is a true 0
                     [7.0, 0.0, 5.0, 0.0, 0.0, 0.0],       # (0, 2): nothing but the held columns -> no counted entry
                     [3.0, -1.0, 3.0, 2.0, 8.0, -0.02]])
    learned = np.array([[2.0, -50.0, -4.0, 60.0, -0.1, 5.0],
                        [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                        [-70.0, 1.0, -9.0, 4.0, 80.0, 0.04]])
    s = phoenix_amd.epistasis_recovery_scores(pairs, true, learned)
    assert isinstance(s, phoenix_amd.EpistasisRecoveryScores) and isinstance(s.per_pair, phoenix_amd.EpistasisPerPair)
    assert s.n_entries == 7 and s.per_pair.n_entries.tolist() == [3, 0, 4] and s.per_pair.n_entries.dtype == np.int64
    t = np.array([1.0, -2.0, 0.05, -1.0, 3.0, 2.0, -0.02])
    l = np.array([2.0, -4.0, -0.1, 1.0, -9.0, 4.0, 0.04])
    assert (s.sign_agreement, s.pearson, s.spearman, s.slope) == recovery_scores(t, l)
    assert s.sign_agreement == 3 / 7
    assert all(np.isnan(x[1]) for x in s.per_pair[1:])                      # the pair without a counted entry: all NaN
    for k, sl in ((0, slice(0, 3)), (2, slice(3, 7))):                      # each row: recovery_scores of its counted entries
        assert tuple(x[k] for x in s.per_pair[1:]) == recovery_scores(t[sl], l[sl]), k
    # min_effect: entries at or below it go (0.05 and -0.02; an entry of exactly min_effect too)
    m = phoenix_amd.epistasis_recovery_scores(pairs, true, learned, min_effect=0.05)
    assert m.n_entries == 5 and m.per_pair.n_entries.tolist() == [2, 0, 3]
    assert m.per_pair.sign_agreement[0] == 1.0 and m.per_pair.slope[0] == 2.0 and m.per_pair.pearson[0] == 1.0
    same = phoenix_amd.epistasis_recovery_scores(pairs, true, true.copy())
    assert (same.sign_agreement, same.pearson, same.spearman, same.slope) == (1.0, 1.0, 1.0, 1.0)
    none = phoenix_amd.epistasis_recovery_scores(pairs, torch.from_numpy(true), torch.from_numpy(learned), min_effect=100.0)
    assert none.n_entries == 0 and all(np.isnan(x) for x in none[1:5]) and np.isnan(none.per_pair.pearson).all()
    assert none.per_pair.n_entries.tolist() == [0, 0, 0]
    for bad in ([(1, 3), (0, 2)], [(1, 3), (0, 2), (4, 6)], [(1, 3), (0, 2), (4,)]):
        with pytest.raises(ValueError, match="epistasis_recovery_scores"):
            phoenix_amd.epistasis_recovery_scores(bad, true, learned)
    with pytest.raises(ValueError, match="epistasis_recovery_scores"):
        phoenix_amd.epistasis_recovery_scores(pairs, true, learned, min_effect=-1.0)


# --------------------------------------------------------------------------- host-side argument checks
def test_knockouts_check_their_sets_on_the_host():
    sys_, _ = cpu_system(12)
    x0 = torch.zeros(2, 12)
    for kw, exc in ((dict(genes=[0, (1, 2, 3, 4, 5)]), ValueError),                     # 5 genes
                    (dict(genes=[0, (1, -1, -1, -1, -1)]), ValueError),                 # ... padding included
                    (dict(genes=[(1, 2, 1)]), ValueError),                              # a gene twice
                    (dict(genes=[(3, 3)], value=[(0.0, 1.0)]), ValueError),
                    (dict(genes=[0, (1, 2)], value=[0.0, (1.0, 2.0, 3.0)]), ValueError),      # a level list of the wrong length
                    (dict(genes=[0, (1, 2)], value=[0.0, (1.0,)]), ValueError),
                    (dict(genes=[0, (1, 2)], value=[0.0]), ValueError),                 # one level list for two calls
                    (dict(genes=[(0, 12)]), ValueError), (dict(genes=[(0, -2)]), ValueError),
                    (dict(genes=[(0, 0.5)]), TypeError), (dict(genes=[(0, True)]), TypeError),
                    (dict(genes=[(0, 1)], value=[(0.0, float("inf"))]), ValueError),
                    (dict(genes=[(0, 1)], dt_max=0.0), ValueError), (dict(genes=[(0, 1)], times=[]), ValueError)):
        kw = dict(dict(times=[0.0, 0.1]), **kw)
        with pytest.raises(exc, match="knockouts"):
            sys_.knockouts(x0, **kw)
    with pytest.raises(ValueError, match="x0 must be"):
        sys_.knockouts(torch.zeros(2, 11), [0.0, 0.1], [(0, 1)])
    for genes, value in (([(0, 1), -1, (), 5], 0.0), ([(0, 1, 2, 11)], [(0.0, 1.0, 2.0, 3.0)]),
                         (np.array([[0, 1], [2, -1]]), np.array([[0.0, 1.0], [2.0, np.nan]]))):
        with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):      # good sets: the next thing is the GPU
            sys_.knockouts(x0, [0.0, 0.1], genes, value)


@pytest.mark.parametrize("kw,exc", [(dict(), ValueError), (dict(pairs=[(0, 1), (2, 2)]), ValueError),
                                    (dict(pairs=[(0, 1), (1, 0)]), ValueError), (dict(genes=[0, 1, 2], value=[0.0, 1.0]), ValueError),
                                    (dict(genes=[0]), ValueError), (dict(genes=[0, 0]), ValueError), (dict(genes=[0, 12]), ValueError),
                                    (dict(pairs=[]), ValueError), (dict(pairs=[(0, 1, 2)]), ValueError),
                                    (dict(genes=[0, 1], pairs=[(0, 2)]), ValueError), (dict(genes=[0, 1.5]), TypeError),
                                    (dict(genes=[0, 1], pairs_per_launch=0), ValueError),
                                    (dict(genes=[0, 1], value=float("inf")), ValueError),
                                    (dict(genes=[0, 1], times=[0.5]), ValueError), (dict(genes=[0, 1], dt_max=-1.0), ValueError),
                                    (dict(genes=[0, 1], max_singles_bytes=4 * 10 * 2 * 2 * 12 - 1), ValueError)])
def test_simulator_knockout_pairs_checks_its_arguments_before_a_device_is_needed(kw, exc):
    sys_, _ = cpu_system(12)
    with pytest.raises(exc, match="knockout_pairs"):
        sys_.knockout_pairs(torch.zeros(2, 12), **kw)


def test_simulator_knockout_pairs_has_no_cpu_path():
    sys_, _ = cpu_system(12)
    with pytest.raises(ValueError, match="x0 must be"):
        sys_.knockout_pairs(torch.zeros(2, 11), genes=[0, 1])
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):      # at the size limit: the next thing is the GPU
        sys_.knockout_pairs(torch.zeros(2, 12), genes=[0, 1], max_singles_bytes=4 * 10 * 2 * 2 * 12)


def test_epistasis_recovery_refuses_a_model_of_another_size_without_a_gpu():
    import phoenix_amd
    sys_, _ = cpu_system(12)
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    with pytest.raises(ValueError, match="the model has 16 genes, the system 12"):
        phoenix_amd.epistasis_recovery(net, sys_, torch.zeros(2, 16), genes=[0, 1])
    net = phoenix_amd.ODENet("cpu", 12, neurons=4)
    with pytest.raises(ValueError, match="knockout_pairs"):      # the screen's own argument rules, before any launch
        phoenix_amd.epistasis_recovery(net, sys_, torch.zeros(2, 12))
