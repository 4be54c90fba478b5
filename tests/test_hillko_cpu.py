"""CPU-only checks of the Hill simulator's knockout screens (phx_hill_knockouts, include/phoenix_hip.h;
`HillSystem.knockouts` / `knockout_effects`, `knockout_recovery`): the symbol exists, every refusal answers before a device
call -- and the numpy restatements that tests/test_hillko_gpu.py holds the kernel to (`rates_reference`,
`knockouts_reference`) are themselves held to the oracle's evaluation of the expression strings, to a case worked by hand, to
the "input gene" form of a clamp and to the reachability structure of the network; `knockout_recovery_scores` on planted
arrays."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_abi_cpu import _declared_symbols
from test_simulator_cpu import synthetic_network, synthetic_states

BAD_ARG = 4
TIMES, DT_MAX = (0.0, 0.3, 0.35, 1.05), 0.1       # the rounding-sensitive sub-step counts of tests/test_simulator_gpu.py


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def cpu_system(N):
    from phoenix_amd.simulator import HillSystem
    names, exprs, info = synthetic_network(N)
    return HillSystem(names, exprs, device="cpu"), info


def descendants(system, g):
    """the genes whose rate depends on gene g directly or through others (`jacobian_pattern()`, graph search from g), as a
    bool [N]; g itself only where a cycle leads back to it"""
    pat = system.jacobian_pattern()
    targets_of = {}
    for r, t in zip(pat.regulator.tolist(), pat.target.tolist()):
        if r != t:
            targets_of.setdefault(r, []).append(t)
    seen, todo = np.zeros(system.N, bool), [g]
    while todo:
        for t in targets_of.get(todo.pop(), ()):
            if not seen[t]:
                seen[t] = True
                todo.append(t)
    return seen


def untouched(system, g):
    """bool [N]: the genes a clamp of g cannot change -- neither g nor a descendant of g (g < 0: none is touched)"""
    if g < 0:
        return np.ones(system.N, bool)
    keep = ~descendants(system, g)
    keep[g] = False
    return keep


def gene_without_descendants(system):
    return next(g for g in range(system.N) if not descendants(system, g).any())


def gene_with_descendants(system, info):
    """the first regulated gene that reaches other genes and leaves others alone"""
    return next(g for g in range(system.N) if not info["is_input"][g] and untouched(system, g).any()
                and (descendants(system, g) & (np.arange(system.N) != g)).any())


# --------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_hill_knockouts", "phx_debug_hill_knockouts_kpt"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change


def test_calls_per_workgroup_follow_the_slot_budget(monkeypatch):
    _, lib = _lib()
    kpt = lib.phx_debug_hill_knockouts_kpt
    monkeypatch.delenv("PHX_HILLKO_KPT", raising=False)
    shipped = kpt(350)
    assert shipped in (1, 2, 4, 8) and kpt(1) == kpt(1024) == shipped
    for n, room in ((1025, 4), (2048, 4), (2049, 2), (4096, 2), (4097, 1), (8192, 1)):
        assert kpt(n) == min(shipped, room), n
    assert kpt(0) == 0 and kpt(8193) == 0
    for want in (1, 2, 4, 8):
        monkeypatch.setenv("PHX_HILLKO_KPT", str(want))
        assert kpt(350) == want and kpt(1025) == min(want, 4) and kpt(8192) == 1
    monkeypatch.setenv("PHX_HILLKO_KPT", "3")           # not a group size: the shipped one
    assert kpt(350) == shipped


def _call(lib, code=0x1000, off=0x2000, len_=0x3000, consts=0x4000, x0=0x5000, times=0x6000, T=4, dt_max=0.1, genes=(0, -1, 7),
          values=(0.0, 0.0, 1.7), K=None, out=0x7000, B=3, N=8):
    """phx_hill_knockouts with made-up device addresses: only calls that must return before touching the device"""
    g = None if genes is None else (C.c_int * len(genes))(*genes)
    v = None if values is None else (C.c_float * len(values))(*values)
    K = (len(genes) if genes is not None else 3) if K is None else K
    return lib.phx_hill_knockouts(code, off, len_, consts, x0, times, T, dt_max, g, v, K, out, B, N, None)


def test_refusals_with_nothing_launched():
    _, lib = _lib()
    for name in ("code", "off", "len_", "consts", "x0", "times", "genes", "values", "out"):
        assert _call(lib, **{name: None}) == BAD_ARG, name
    for name in ("B", "N", "K", "T"):
        assert _call(lib, **{name: 0}) == BAD_ARG and _call(lib, **{name: -1}) == BAD_ARG, name
    for dt in (0.0, -0.1, float("nan")):
        assert _call(lib, dt_max=dt) == BAD_ARG, dt
    assert _call(lib, N=8193, genes=(0, -1, 8192)) == BAD_ARG
    assert _call(lib, genes=(0, -1, 8)) == BAD_ARG          # N = 8: the last gene is 7
    assert _call(lib, genes=(0, -2, 7)) == BAD_ARG          # -1 alone means none
    for bad in (float("inf"), -float("inf"), float("nan")):
        assert _call(lib, values=(0.0, bad, 1.7)) == BAD_ARG, bad
    assert _call(lib, B=(1 << 31) // 3 + 1) == BAD_ARG      # K * B = 3 B does not fit an int
    assert _call(lib, genes=(0, 1), values=(0.0, 0.0), B=1 << 30) == BAD_ARG


# --------------------------------------------------------------------------- the numpy restatements
def test_rates_reference_against_the_oracle():
    from oracle import hill_oracle
    from phoenix_amd.simulator import rates_reference
    names, exprs, info = synthetic_network(1025)
    sys_, _ = cpu_system(1025)
    x = synthetic_states(1025, 4, info)
    assert np.any(x <= 0) and np.any(x > 1)
    want = hill_oracle.compile_rhs(names, exprs, fact=hill_oracle.fAct0)(x)
    got = rates_reference(sys_, x)
    assert got.dtype == np.float64 and got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    print("rates_reference against the oracle, N = 1025: max abs err %.2e" % err)
    assert err < 1e-12
    assert np.all(got[:, sys_.is_input] == 0)
    # ... and it is the interpreter of the oracle gene by gene, bit for bit (genes of one opcode sequence side by side)
    one_by_one = hill_oracle.interpret_programs(sys_.code_host, sys_.consts_host, sys_.off_host, sys_.len_host, x.astype(np.float64))
    assert np.array_equal(got, one_by_one)
    got32 = rates_reference(sys_, x, dtype=np.float32)
    assert got32.dtype == np.float32 and np.max(np.abs(got32 - want)) < 5e-5
    assert rates_reference(sys_, x.reshape(2, 2, 1025)).shape == (2, 2, 1025)


def test_knockouts_reference_on_a_case_worked_by_hand():
    """A' = 0.5 - A, B' = A - B with A held at c: B(t) = c + (B0 - c) e^-t; unperturbed, A(t) = 0.5 + (A0 - 0.5) e^-t"""
    from phoenix_amd.simulator import HillSystem, knockouts_reference
    sys_ = HillSystem(["A", "B"], ["0.5 - A", "A - B"], device="cpu")
    x0 = np.array([[0.9, 0.2], [0.1, 1.4]])
    times, c = np.array([0.0, 0.5, 1.3, 1.31]), 0.3
    out = knockouts_reference(sys_, x0, times, [0, -1], [c, 0.0], 0.01)
    assert out.shape == (4, 2, 2, 2) and out.dtype == np.float64
    e = np.exp(-times)[:, None]
    assert np.all(out[:, 0, :, 0] == c)
    assert np.max(np.abs(out[:, 0, :, 1] - (c + (x0[None, :, 1] - c) * e))) < 1e-8
    assert np.max(np.abs(out[:, 1, :, 0] - (0.5 + (x0[None, :, 0] - 0.5) * e))) < 1e-8
    assert np.array_equal(out[0, 1], x0) and np.array_equal(out[0, 0], np.array([[c, 0.2], [c, 1.4]]))
    # decreasing times integrate back: the last state of the way out returns to the first
    back = knockouts_reference(sys_, out[-1, 0], times[::-1], [0], [c], 0.01)
    assert np.max(np.abs(back[-1, 0] - out[0, 0])) < 1e-8


def test_a_clamp_is_an_input_gene_bit_for_bit():
    from phoenix_amd.simulator import HillSystem, knockouts_reference
    names, exprs, info = synthetic_network(65)
    sys_, _ = cpu_system(65)
    g, v = gene_with_descendants(sys_, info), 1.7
    x0 = synthetic_states(65, 3, info, seed=4)
    held = knockouts_reference(sys_, x0, TIMES, [g], [v], DT_MAX)[:, 0]
    as_input = HillSystem(names, [e if i != g else "input gene" for i, e in enumerate(exprs)], device="cpu")
    x1 = x0.astype(np.float64)
    x1[:, g] = v
    want = knockouts_reference(as_input, x1, TIMES, [-1], [0.0], DT_MAX)[:, 0]
    assert np.array_equal(held, want) and np.all(held[:, :, g] == v)
    free = knockouts_reference(sys_, x0, TIMES, [-1], [0.0], DT_MAX)[:, 0]
    assert not np.array_equal(held, free)


def test_a_clamp_moves_its_descendants_and_nothing_else():
    from phoenix_amd.simulator import knockouts_reference
    sys_, info = cpu_system(65)
    x0 = synthetic_states(65, 3, info, seed=4)
    g, lone = gene_with_descendants(sys_, info), gene_without_descendants(sys_)
    genes, values = [-1, g, g, lone, lone], [0.0, 0.0, 1.7, 0.0, 1.7]
    ref = knockouts_reference(sys_, x0, TIMES, genes, values, DT_MAX)
    scale = float(np.max(np.abs(ref)))
    assert descendants(sys_, g).any() and untouched(sys_, lone).sum() == 64
    for k in range(1, 5):
        keep = untouched(sys_, genes[k])
        assert np.array_equal(ref[:, k][:, :, keep], ref[:, 0][:, :, keep]), k      # bit for bit
        assert np.all(ref[:, k, :, genes[k]] == values[k])
        moved = np.abs(ref[:, k] - ref[:, 0])[:, :, descendants(sys_, genes[k]) & (np.arange(65) != genes[k])]
        print("gene %d at %.1f: %d untouched genes, descendants move by %.2e of max|ref|"
              % (genes[k], values[k], keep.sum(), moved.max() / scale if moved.size else 0.0))
        if genes[k] == g:
            assert moved.max() > 1e-3 * scale


# --------------------------------------------------------------------------- host-side argument checks
def test_knockouts_check_their_arguments_on_the_host():
    sys_, info = cpu_system(12)
    x0 = torch.zeros(2, 12)
    for kw, exc in ((dict(genes=[0, 12]), ValueError), (dict(genes=[-2]), ValueError), (dict(genes=[0.5]), TypeError),
                    (dict(genes=[True]), TypeError), (dict(genes=[]), ValueError), (dict(genes=[0, 1], value=[0.0]), ValueError),
                    (dict(genes=[0], value=float("inf")), ValueError), (dict(genes=[0], dt_max=0.0), ValueError),
                    (dict(genes=[0], times=[]), ValueError)):
        kw = dict(dict(times=[0.0, 0.1]), **kw)
        with pytest.raises(exc, match="knockouts"):
            sys_.knockouts(x0, **kw)
    with pytest.raises(ValueError, match="x0 must be"):
        sys_.knockouts(torch.zeros(2, 11), [0.0, 0.1], [0])
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        sys_.knockouts(x0, [0.0, 0.1], [0, -1])
    for kw, exc in ((dict(genes=[-1]), ValueError), (dict(genes=[0], genes_per_launch=0), ValueError),
                    (dict(genes=[0], times=[0.5]), ValueError)):
        with pytest.raises(exc, match="knockout_effects"):
            sys_.knockout_effects(x0, **kw)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        sys_.knockout_effects(x0, genes=[0, 3])


# --------------------------------------------------------------------------- recovery statistics
def test_knockout_recovery_scores_on_planted_arrays():
    import phoenix_amd
    from phoenix_amd.analysis import recovery_scores
    genes = [1, 0, 2]
    true = np.array([[1.0, 9.0, -2.0, 0.0, 0.05],       # gene 1 held: column 1 is left out, column 3 is a true 0
                     [7.0, 0.0, 0.0, 0.0, 0.0],         # gene 0 held: nothing else moves -> no counted entry
                     [0.5, -1.0, 3.0, 2.0, -0.02]])
    learned = np.array([[2.0, -50.0, -4.0, 5.0, -0.1],
                        [1.0, 1.0, 1.0, 1.0, 1.0],
                        [1.0, 1.0, -9.0, 4.0, 0.04]])
    s = phoenix_amd.knockout_recovery_scores(genes, true, learned)
    assert s.n_entries == 7 and s.per_gene.n_entries.tolist() == [3, 0, 4]
    t = np.array([1.0, -2.0, 0.05, 0.5, -1.0, 2.0, -0.02])
    l = np.array([2.0, -4.0, -0.1, 1.0, 1.0, 4.0, 0.04])
    assert (s.sign_agreement, s.pearson, s.spearman, s.slope) == recovery_scores(t, l)
    assert s.sign_agreement == 4 / 7 and math.isclose(s.slope, float(t @ l) / float(t @ t))
    assert s.per_gene.sign_agreement[0] == 2 / 3 and s.per_gene.sign_agreement[2] == 2 / 4
    assert all(np.isnan(x[1]) for x in s.per_gene[1:])                      # the knockout without a counted entry
    assert (s.per_gene.sign_agreement[2], s.per_gene.pearson[2], s.per_gene.spearman[2], s.per_gene.slope[2]) == \
        recovery_scores(t[3:], l[3:])
    # min_effect: the two small entries go, the rest is a perfect doubling except one sign
    m = phoenix_amd.knockout_recovery_scores(genes, true, learned, min_effect=0.1)
    assert m.n_entries == 5 and m.per_gene.n_entries.tolist() == [2, 0, 3]
    assert m.per_gene.sign_agreement[0] == 1.0 and math.isclose(m.per_gene.slope[0], 2.0) and m.per_gene.pearson[0] == 1.0
    # learned == true: 1, 1, 1, 1 (pooled and for every knockout with two or more counted entries)
    same = phoenix_amd.knockout_recovery_scores(genes, true, true.copy())
    assert (same.sign_agreement, same.pearson, same.spearman, same.slope) == (1.0, 1.0, 1.0, 1.0)
    for i in (0, 2):
        assert [x[i] for x in same.per_gene[1:]] == [1.0, 1.0, 1.0, 1.0]
    # tensors are taken as they come; everything below the bar: NaNs throughout
    none = phoenix_amd.knockout_recovery_scores(genes, torch.from_numpy(true), torch.from_numpy(learned), min_effect=100.0)
    assert none.n_entries == 0 and all(np.isnan(x) for x in none[1:5]) and np.isnan(none.per_gene.pearson).all()
    with pytest.raises(ValueError, match="knockout_recovery_scores"):
        phoenix_amd.knockout_recovery_scores([0, 1], true, learned)
    with pytest.raises(ValueError, match="knockout_recovery_scores"):
        phoenix_amd.knockout_recovery_scores([0, 1, 5], true, learned)


def test_knockout_recovery_refuses_a_model_of_another_size_without_a_gpu():
    import phoenix_amd
    sys_, _ = cpu_system(12)
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    with pytest.raises(ValueError, match="the model has 16 genes, the system 12"):
        phoenix_amd.knockout_recovery(net, sys_, torch.zeros(2, 16), genes=[0])
