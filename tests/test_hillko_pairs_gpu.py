"""phx_hill_knockout_sets (csrc/phx_hillko.hip; `HillSystem.knockouts` with held sets, `HillSystem.knockout_pairs`,
`epistasis_recovery`) on the synthetic networks of tests/test_simulator_cpu.py against `knockouts_reference` in float64
(held to the "input gene" form of a set and to a case worked by hand in tests/test_hillko_pairs_cpu.py).  Run with `-m gpu`.

Bars, from tests/test_hillko_gpu.py: TRAJ_BAR = 1e-5 max-norm relative on trajectories, per call and per gene; 2 TRAJ_BAR
scale absolute on shift and magnitude (a difference of two trajectory entries, each within the bar, and means of such);
4 TRAJ_BAR scale on interaction, interaction magnitude and both scores: d_ab - (d_a + d_b) combines four trajectory entries,
each within the bar.  Everything structural is bitwise: held columns, out[0], a set against its other order, a 1-entry set
against the single-gene entry point, what no held gene reaches against the -1 call, what only one gene of a pair reaches
against that gene's own call -- and so the exact zeros of an interaction."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_hillko_cpu import DT_MAX, TIMES, descendants, gene_without_descendants, untouched
from test_hillko_gpu import TRAJ_BAR, hold, reference, run, system
from test_hillko_pairs_cpu import PAIR
from test_knockout_pairs_cpu import reference64_pairs
from test_simulator_cpu import synthetic_states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def members(entry):
    """the held genes of a call: an int (-1: none) or a sequence with -1 padding"""
    return [g for g in (entry if isinstance(entry, (tuple, list)) else (entry,)) if g >= 0]


def levels_of(entry, value):
    held = members(entry)
    return dict(zip(held, value if isinstance(value, (tuple, list)) else (value,) * len(held)))


def set_calls(sys_, info):
    """the K = 12 calls of the cases -> (genes, values, names): nothing held as -1 and as (); a gene as an int and as a 1-tuple;
    a pair that meets in a gate, in both orders, at distinct levels; sets of 3 and 4 with the last gene of the network and an
    input gene at a negative level (its targets see fAct at TF <= 0); that input gene alone; and a gene that reaches some of
    the network (held high: a level of 0 is where fAct is 0 anyway) beside one that reaches nothing, with the two alone"""
    N = sys_.N
    inputs = np.flatnonzero(info["is_input"]).tolist()
    inp = next((g for g in inputs if descendants(sys_, g).any()), inputs[0])
    lone = gene_without_descendants(sys_)
    reach = {g: int(descendants(sys_, g).sum()) for g in range(1, 33) if not info["is_input"][g] and untouched(sys_, g).any()}
    far = max(reach, key=reach.get)      # of the first genes the one that reaches most of the network, and not all of it
    a, b = next(p for p in sys_.coregulator_pairs() if not (set(p) & {inp, lone, far, 0, N - 1}))
    genes = [-1, (), 0, (0,), (a, b), (b, a), (inp, N - 1, 0), (N - 1, lone, inp, far), inp, (far, lone), far, lone]
    values = [0.0, 0.0, 1.7, 1.7, (0.0, 0.4), (0.4, 0.0), (-0.15, 0.4, 1.7), (0.4, 0.9, -0.15, 1.1), -0.15, (1.1, 0.9), 1.1, 0.9]
    return genes, values, dict(inp=inp, lone=lone, far=far, a=a, b=b)


NARROW = [0, 2, 3, 4, 5, 9, 10]      # the calls of width <= 2: on their own they run at the width-2 instantiation
PLAIN = [0, 2, 8, 10, 11]            # the int entries: a list of them goes through phx_hill_knockouts


@functools.lru_cache(maxsize=None)
def set_case(N):
    """(system, info, x0, times, genes, values, names, reference, results of the whole list / NARROW / PLAIN) at N genes:
    computed once, shared, read only"""
    sys_, info = system(N)
    B, times = (1, TIMES[:3]) if N == 8192 else (3, TIMES)      # the largest network: as in tests/test_hillko_gpu.py
    x0 = synthetic_states(N, B, info, seed=4)
    genes, values, names = set_calls(sys_, info)
    ref = reference(sys_, x0, times, genes, values)
    got = run(sys_, x0, times, genes, values)
    narrow = run(sys_, x0, times, [genes[k] for k in NARROW], [values[k] for k in NARROW])
    plain = run(sys_, x0, times, [genes[k] for k in PLAIN], [values[k] for k in PLAIN])
    for arr in (x0, ref, got, narrow, plain):
        arr.setflags(write=False)
    return sys_, info, x0, times, genes, values, names, ref, got, narrow, plain


@pytest.mark.parametrize("N", [63, 65, 1025, 8192])
def test_sets_against_float64(dev, N):
    """one wave minus / plus one gene; 1025: two genes per thread and gene 1024 held in a set of 3 and of 4; 8192: eight genes
    per thread.  The whole list runs at width 4, its calls of width <= 2 again at width 2"""
    sys_, info, x0, times, genes, values, names, ref, got, narrow, plain = set_case(N)
    assert info["is_input"][names["inp"]] and any(N - 1 in members(g) and len(g) == w for w in (3, 4) for g in genes[6:8])
    assert sorted(len(members(g)) for g in genes) == [0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 3, 4]
    hold("N=%d K=%d width 4" % (N, len(genes)), got, ref)
    hold("N=%d K=%d width 2" % (N, len(NARROW)), narrow, ref[:, NARROW])
    hold("N=%d K=%d single-gene entry" % (N, len(PLAIN)), plain, ref[:, PLAIN])


@pytest.mark.parametrize("N", [63, 65, 1025, 8192])
def test_sets_structure_is_bitwise(dev, N):
    sys_, info, x0, times, genes, values, names, ref, got, narrow, plain = set_case(N)
    scale = float(np.max(np.abs(ref)))
    for k, (entry, value) in enumerate(zip(genes, values)):
        want0 = x0.copy()
        for g, v in levels_of(entry, value).items():
            want0[:, g] = v
            assert np.all(got[:, k, :, g] == np.float32(v)), (k, g)             # every held column, at every time
        assert np.array_equal(got[0, k], want0), k                               # out[0]: x0 with those columns replaced
        keep = np.ones(N, bool)
        for g in members(entry):
            keep &= untouched(sys_, g)
        assert np.array_equal(got[:, k][:, :, keep], got[:, 0][:, :, keep]), k   # what no held gene reaches: the -1 call
    assert np.array_equal(got[:, 1], got[:, 0])                                  # () is -1
    assert np.array_equal(got[:, 3], got[:, 2])                                  # a 1-tuple is the int, beside wider sets ...
    assert np.array_equal(got[:, PLAIN], plain)                                  # ... and through the single-gene entry point
    assert np.array_equal(got[:, NARROW], narrow)                                # the width a call runs at leaves no trace
    assert np.array_equal(got[:, 4], got[:, 5]) and not np.array_equal(got[:, 4], got[:, 0])      # (a, b) is (b, a)
    # a gene reached by one gene of a pair and not by the other: the bits of that gene's own call
    far, lone = names["far"], names["lone"]
    only_far = descendants(sys_, far) & ~descendants(sys_, lone)
    only_far[[far, lone]] = False
    assert only_far.any() and np.array_equal(got[:, 9][:, :, only_far], got[:, 10][:, :, only_far])
    rest = np.arange(N) != far
    assert np.array_equal(got[:, 9][:, :, rest & ~only_far], got[:, 11][:, :, rest & ~only_far])   # ... and the other way round
    moved = float(np.abs(ref[:, 10] - ref[:, 0])[:, :, only_far].max())
    print("N=%d: gene %d reaches %d genes that gene %d does not; the reference moves one by %.2e of max|ref|"
          % (N, far, only_far.sum(), lone, moved / scale))
    assert moved > 100 * TRAJ_BAR * scale                                        # not vacuous: they do move


def test_a_nan_level_on_a_pad_is_not_looked_at(dev):
    """the call tests/test_hillko_pairs_cpu.py cannot make with made-up addresses: NaN levels on -1 entries pass the argument
    checks of the entry point itself and leave no trace"""
    from phoenix_amd import _lib, engine
    sys_, info, x0, times, genes, values, names, ref, got, narrow, plain = set_case(65)
    a, b, nan = names["a"], names["b"], float("nan")
    rows, lv = [a, b, -1, -1, 0, -1, -1, -1], [0.0, 0.4, nan, nan, 1.7, nan, nan, nan]      # [K = 4, width = 2]
    x2, t64 = torch.from_numpy(x0.copy()).to(dev), torch.tensor(times, dtype=torch.float64, device=dev)
    out = torch.empty((len(times), 4 * 3, 65), dtype=torch.float32, device=dev)
    rc = _lib.load().phx_hill_knockout_sets(*sys_._args(), engine._p(x2), engine._p(t64), len(times), C.c_double(DT_MAX),
                                            (C.c_int * 8)(*rows), (C.c_float * 8)(*lv), 2, 4, engine._p(out), 3, 65,
                                            engine._stream_ptr())
    assert rc == 0
    assert np.array_equal(out.cpu().numpy().reshape(len(times), 4, 3, 65), got[:, [4, 0, 2, 0]])


def test_a_call_does_not_depend_on_its_group(dev):
    """K = 9 calls of mixed widths: full groups and a remainder; a pair beside a duplicate of itself and beside the same pair
    at other levels; all of them in reversed order, and each call alone (where it runs at the width of its own set)"""
    sys_, info = system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    a, b = PAIR
    genes = [(a, b), (a, b), -1, (a, b), (0,), (info["unary"], 7, 33), (info["deep"], 0, 7, 64), (), 33]
    values = [0.0, 0.0, 0.0, (1.7, 0.4), 1.7, (0.4, -0.15, 1.1), (0.0, 0.6, -0.15, 0.4), 0.0, 1.1]
    got = run(sys_, x0, TIMES, genes, values)
    assert np.array_equal(got[:, 0], got[:, 1]) and not np.array_equal(got[:, 0], got[:, 3])
    back = run(sys_, x0, TIMES, genes[::-1], values[::-1])
    assert np.array_equal(back[:, ::-1], got)
    for k in range(9):
        alone = run(sys_, x0, TIMES, genes[k:k + 1], values[k:k + 1])
        assert np.array_equal(alone[:, 0], got[:, k]), k


def test_knockout_pairs_of_the_simulator(dev):
    """`HillSystem.knockout_pairs` in blocks of 2 pairs and in one block against the scoring formulas in float64 on the
    float64 trajectories; exact zeros off the common descendants; not vacuous: (1, 39) interacts at 0.163 max|ref|"""
    sys_, info = system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    lone = gene_without_descendants(sys_)
    pairs = [PAIR, (lone, PAIR[0]), (38, 29), (PAIR[1], 44), (29, lone)]
    genes = sorted(set(g for p in pairs for g in p))
    values = [0.0 if g in PAIR else 0.4 + 0.1 * i for i, g in enumerate(genes)]
    index = {g: i for i, g in enumerate(genes)}
    ia, ib = [index[p[0]] for p in pairs], [index[p[1]] for p in pairs]
    G, K, T = len(genes), len(pairs), len(TIMES)
    ref = reference(sys_, x0, TIMES, [-1] + genes + pairs, [0.0] + values + [(values[i], values[j]) for i, j in zip(ia, ib)])
    scale = float(np.max(np.abs(ref)))
    want = reference64_pairs(ref[:, 0], ref[:, 1:1 + G].reshape(T, G * 3, 65), ref[:, 1 + G:].reshape(T, K * 3, 65), ia, ib, genes)
    common = [descendants(sys_, a) & descendants(sys_, b) for a, b in pairs]
    assert not common[1].any() and not common[4].any() and common[0].any()       # pairs without a common descendant, and with
    assert np.abs(want[4]).max() > 100 * TRAJ_BAR * scale                         # the truth has content ...
    print("largest |mean interaction| of the reference: %.3f of max|ref| (pair %r)"
          % (np.abs(want[4]).max() / scale, pairs[int(np.abs(want[4]).max(axis=1).argmax())]))
    assert np.abs(want[4][0]).max() > 0.1 * scale                                 # ... 0.163 max|ref| for (1, 39)
    x0d = torch.from_numpy(x0.copy()).to(sys_.device)
    results = []
    for per_launch in (2, 64):
        res = sys_.knockout_pairs(x0d, genes, pairs, values, TIMES, DT_MAX, pairs_per_launch=per_launch)
        assert res.pairs == pairs and res.genes == genes and res.singles.genes == genes
        assert res.scores.dtype == np.float32 and res.interaction_scores.shape == (K,) and tuple(res.interaction.shape) == (K, 65)
        got = (res.scores, res.interaction_scores) + tuple(x.cpu().numpy() for x in res[4:8])
        names = ("scores", "interaction_scores", "shift", "magnitude", "interaction", "interaction_magnitude")
        for name, g, w in zip(names, got, want):
            bar = (2 if name in ("shift", "magnitude") else 4) * TRAJ_BAR * scale
            err = float(np.abs(g - w).max())
            print("pairs_per_launch %d: %s err %.2e, bar %.2e" % (per_launch, name, err, bar))
            assert err <= bar, (per_launch, name, err, bar)
        for k, (a, b) in enumerate(pairs):
            zero = ~common[k]
            zero[[a, b]] = False       # the held genes are no targets
            assert np.all(got[4][k, zero] == 0) and np.all(got[5][k, zero] == 0), (k, a, b)      # exactly
        assert res.interaction_scores[1] == 0 and res.interaction_scores[4] == 0 and res.interaction_scores[0] > 0
        one = sys_.knockout_effects(x0d, genes, values, TIMES, DT_MAX)
        assert np.array_equal(res.singles.scores, one.scores) and torch.equal(res.singles.shift, one.shift)
        only = sys_.knockout_pairs(x0d, genes, pairs, values, TIMES, DT_MAX, pairs_per_launch=per_launch, want_matrices=False)
        assert all(x is None for x in only[4:8]) and only.singles.shift is None
        assert np.array_equal(only.scores, res.scores) and np.array_equal(only.interaction_scores, res.interaction_scores)
        results.append(got)
    for x, y in zip(*results):
        assert np.array_equal(x, y)                                               # 2 pairs per launch or all: the same bits
    # genes=: all their pairs, the default time points
    allp = sys_.knockout_pairs(x0d, genes=[1, 39, 29], dt_max=DT_MAX)
    assert allp.pairs == [(1, 39), (1, 29), (39, 29)] and np.all(np.isfinite(allp.interaction_scores))


def test_epistasis_recovery_end_to_end(dev):
    """a random model against the simulator: `true` and `learned` are the two screens called directly, bit for bit, and the
    statistics are `epistasis_recovery_scores` of them; nothing is asked of a random model's quality"""
    import phoenix_amd
    from phoenix_amd.analysis import _average_ranks, _pearson
    N, B = 96, 5
    sys_, info = system(N)
    torch.manual_seed(0)
    net = phoenix_amd.ODENet(dev, N, neurons=8)
    y0 = torch.from_numpy(synthetic_states(N, B, info, seed=4)).to(dev)
    a, b = sys_.coregulator_pairs()[0]
    genes = [a, b, info["unary"], gene_without_descendants(sys_)]
    assert len(set(genes)) == 4
    values = [0.0, 0.0, 0.4, 1.7]
    t = torch.from_numpy(np.arange(0, 1, 0.25))
    rec = phoenix_amd.epistasis_recovery(net, sys_, y0, genes, None, values, t, dt_max=0.05, min_effect=1e-6)
    assert isinstance(rec, phoenix_amd.EpistasisRecovery) and len(rec.pairs) == 6 and rec.pairs[0] == (a, b)
    learned = phoenix_amd.knockout_pairs(net, y0, genes, None, values, t)
    true = sys_.knockout_pairs(y0, genes, None, values, t, 0.05)
    for x, y in ((rec.true, true), (rec.learned, learned)):
        assert x.pairs == y.pairs == rec.pairs and x.genes == y.genes == genes
        assert np.array_equal(x.scores, y.scores) and np.array_equal(x.interaction_scores, y.interaction_scores)
        assert all(torch.equal(p, q) for p, q in zip(x[4:8], y[4:8]))
        assert np.array_equal(x.singles.scores, y.singles.scores) and torch.equal(x.singles.shift, y.singles.shift)
    s = phoenix_amd.epistasis_recovery_scores(rec.pairs, true.interaction, learned.interaction, min_effect=1e-6)
    j = phoenix_amd.epistasis_recovery_scores(rec.pairs, true.shift, learned.shift, min_effect=1e-6)
    same = lambda p, q: p == q or (np.isnan(p) and np.isnan(q))      # noqa: E731
    assert rec.n_entries == s.n_entries > 0 and rec.joint.n_entries == j.n_entries > s.n_entries
    assert all(same(p, q) for p, q in zip(rec[2:6], s[1:5])) and all(same(p, q) for p, q in zip(rec.joint[1:5], j[1:5]))
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(rec.per_pair, s.per_pair))
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(rec.joint.per_pair, j.per_pair))
    lone_pairs = [k for k, p in enumerate(rec.pairs) if genes[3] in p]
    assert len(lone_pairs) == 3 and all(rec.per_pair.n_entries[k] == 0 for k in lone_pairs) and rec.per_pair.n_entries[0] > 0
    want = _pearson(_average_ranks(true.interaction_scores.astype(np.float64)),
                    _average_ranks(learned.interaction_scores.astype(np.float64)))
    assert same(rec.scores_spearman, want) and -1.0 <= rec.scores_spearman <= 1.0
    print("epistasis_recovery of a random model: %d entries, sign %.3f pearson %.3f spearman %.3f slope %.3g, scores %.3f"
          % (rec.n_entries, rec.sign_agreement, rec.pearson, rec.spearman, rec.slope, rec.scores_spearman))
