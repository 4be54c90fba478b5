"""CPU-side checks of the pathway permutation test (`pathway_permutation_test`, phx_pathway_permutations of
include/phoenix_hip.h): `perm_ref` / `pathway_ref`, the numpy mirror of the contract that the GPU tests compare the kernel
with, held to theory (a uniform rank, the moments of sampling without replacement); the host functions
`consolidate_gene_scores`, `read_pathways` (golden G24), `write_permutation_table` and `PermutationTest.merge`; and the
argument checks of the C entry points and the Python callers, none of which needs a device."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5
GOLD = np.uint64(0x9E3779B97F4A7C15)


# --------------------------------------------------------------------------- the mirror (the reference, not code under test)
def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys_ref(seed, r, N):
    """key[..., g] of permutations `r` (an integer or an array of them): uint64 arithmetic modulo 2^64"""
    g = np.arange(N, dtype=np.uint64)
    c = (np.asarray(r, dtype=np.uint64)[..., None] << np.uint64(14)) | g
    with np.errstate(over="ignore"):
        z = _mix(_mix(np.uint64(seed) + GOLD * (c + np.uint64(1))))
    return (z & ~np.uint64(0x3FFF)) | g


def perm_ref(seed, r, N):
    """order_r: the genes sorted by ascending key (permuted_r[g] = scores[order_r[g]])"""
    return np.argsort(keys_ref(seed, r, N), axis=-1, kind="stable").astype(np.int64)


def membership(ptr, idx, N):
    M = np.zeros((len(ptr) - 1, N), dtype=np.float64)
    for p in range(len(ptr) - 1):
        M[p, idx[ptr[p]:ptr[p + 1]]] = 1.0
    return M


def pathway_ref(scores, ptr, idx, seed, first, n_perm, chunk=512, near=False):
    """(base float64 [P], count int64 [P], s1, s2 float64 [P]) of the contract: fp64 sums as a dense 0/1 membership
    product (exact on dyadic scores, whatever the order).  `near=True`: the function also returns how many (r, p) have
    |x_r - base| <= 2 (m - 1) 2^-53 sum |scores| over the m > 1 members of the pathway: the comparisons base < x_r that two
    fp64 summation orders, each within (m - 1) 2^-53 sum |scores| of the exact sums, may decide differently (a one-member
    pathway has nothing to round)."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    N, P = s.shape[0], len(ptr) - 1
    M = membership(ptr, idx, N)
    base = M @ s
    count, s1, s2, close = np.zeros(P, np.int64), np.zeros(P), np.zeros(P), 0
    m = M.sum(axis=1)
    bound = 2 * (m - 1) * 2.0 ** -53 * (M @ np.abs(s))
    for r0 in range(first, first + n_perm, chunk):
        r = np.arange(r0, min(r0 + chunk, first + n_perm), dtype=np.uint64)
        x = s[perm_ref(seed, r, N)] @ M.T                      # [Rc, P]
        d = x - base
        count += (base < x).sum(axis=0)
        s1 += d.sum(axis=0)
        s2 += (d * d).sum(axis=0)
        if near:
            close += int(((np.abs(d) <= bound) & (m > 1)).sum())
    return (base, count, s1, s2, close) if near else (base, count, s1, s2)


def stats_ref(base, count, s1, s2, R):
    """the reference's columns from the raw sums: (z, mean, sd, p)"""
    mean = base + s1 / R
    sd = np.sqrt(np.maximum(0.0, (s2 - s1 * s1 / R) / (R - 1)))
    z = np.where(sd > 0, (base - mean) / np.where(sd > 0, sd, 1.0), 0.0)
    return z, mean, sd, count / R


def table_ref(names, z, mean, sd, p):
    lines = ['"pathway","phnx_z_score","mean_path_score","sd_path_score","phnx_p_val"\n']
    for k in np.argsort(-z, kind="stable"):
        lines.append('"%s",%.15g,%.15g,%.15g,%.15g\n' % (names[k], z[k], mean[k], sd[k], p[k]))
    return "".join(lines)


def grid_scores(rng, N):
    """scores k / 64, k in [-64, 64], with ties: every sum of them and of their squares below is exact in float64"""
    return (rng.integers(-64, 65, N) / 64.0).astype(np.float32)


def pathways_of_sizes(rng, N, sizes):
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    idx = np.concatenate([rng.permutation(N)[:m] for m in sizes] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, idx


NINE = (0, 1, 2, 3, 17, 64, 65, 129, 130)       # the sizes of the N = 130 case, shared with tests/test_pathways_gpu.py


def case_130():
    rng = np.random.default_rng(130)
    scores = grid_scores(rng, 130)
    ptr, idx = pathways_of_sizes(rng, 130, NINE)
    return scores, ptr, idx


ORDINARY = (1, 2, 3, 17, 64, 65, 127)           # the sizes of the case with ordinary scores: all below N = 130
ORDINARY_SEED = 13


def case_ordinary():
    """scores from torch.rand and pathways for which no permutation of ORDINARY_SEED in [0, 4096) brings a sum within
    rounding of its base (test_the_ordinary_case_has_no_comparison_within_rounding)"""
    scores = torch.rand(130, generator=torch.Generator().manual_seed(130)).numpy()
    ptr, idx = pathways_of_sizes(np.random.default_rng(131), 130, ORDINARY)
    return scores, ptr, idx


_cache = {}


def ref_ordinary():
    if "ord" not in _cache:
        scores, ptr, idx = case_ordinary()
        _cache["ord"] = pathway_ref(scores, ptr, idx, ORDINARY_SEED, 0, 4096, near=True)
    return _cache["ord"]


def ref_130():
    """the mirror on the N = 130 case, seed 7, permutations [0, 4096): computed once"""
    if "r130" not in _cache:
        scores, ptr, idx = case_130()
        _cache["r130"] = pathway_ref(scores, ptr, idx, 7, 0, 4096)
    return _cache["r130"]


# --------------------------------------------------------------------------- the mirror against theory
def test_keys_are_distinct_and_order_is_a_permutation():
    for seed, r, N in ((0, 0, 1), (0, 0, 2), (7, 5, 130), (2 ** 64 - 1, 2 ** 50 - 1, 16384), (3, 2 ** 40, 1025)):
        k = keys_ref(seed, r, N)
        assert k.dtype == np.uint64 and len(np.unique(k)) == N
        assert np.array_equal(k & np.uint64(0x3FFF), np.arange(N, dtype=np.uint64))
        order = perm_ref(seed, r, N)
        assert np.array_equal(np.sort(order), np.arange(N))
    # a permutation is a function of (seed, r) alone: the batched form is the single one, row by row
    many = perm_ref(7, np.arange(10, 14, dtype=np.uint64), 130)
    for j, r in enumerate(range(10, 14)):
        assert np.array_equal(many[j], perm_ref(7, r, 130))
    assert not np.array_equal(perm_ref(7, 0, 130), perm_ref(8, 0, 130))
    assert not np.array_equal(perm_ref(7, 0, 130), perm_ref(7, 1, 130))
    # the all-ones pad word of the kernel's sort is above every key of a gene when anything is padded (N < 16384)
    assert keys_ref(2 ** 64 - 1, 2 ** 50 - 1, 16383).max() < np.uint64(2 ** 64 - 1)


def test_the_rank_of_gene_0_is_uniform():
    N, R = 130, 20000
    order = perm_ref(3, np.arange(R, dtype=np.uint64), N)
    e = R / N
    for what, seen in (("the gene at position 0", order[:, 0]), ("the position of gene 0", np.argmax(order == 0, axis=1))):
        chi2 = float(((np.bincount(seen, minlength=N) - e) ** 2 / e).sum())
        print("%s over %d permutations: chi^2 = %.1f at %d degrees of freedom" % (what, R, chi2, N - 1))
        assert chi2 < 184.38                                  # the 99.9 % quantile of chi^2(129)


def test_null_moments_are_those_of_sampling_without_replacement():
    scores, ptr, idx = case_130()
    base, count, s1, s2 = ref_130()
    N, R = 130, 4096
    z, mean, sd, p = stats_ref(base, count, s1, s2, R)
    s = scores.astype(np.float64)
    mu, var = s.mean(), s.var()
    for k, m in enumerate(NINE):
        if m in (0, 130):
            continue
        t_mean, t_sd = m * mu, np.sqrt(m * (N - m) / (N - 1) * var)
        # standard errors of a sample mean and (normal approximation) of a sample standard deviation over R draws
        se_mean, se_sd = t_sd / np.sqrt(R), t_sd / np.sqrt(2 * (R - 1))
        print("m = %3d  mean %.4f (theory %.4f, %.2f se)  sd %.4f (theory %.4f, %.2f se)"
              % (m, mean[k], t_mean, (mean[k] - t_mean) / se_mean, sd[k], t_sd, (sd[k] - t_sd) / se_sd))
        assert abs(mean[k] - t_mean) < 5 * se_mean and abs(sd[k] - t_sd) < 5 * se_sd
        assert 0 < count[k] < R


def test_full_and_empty_pathways_have_no_spread():
    base, count, s1, s2 = ref_130()
    z, mean, sd, p = stats_ref(base, count, s1, s2, 4096)
    scores = case_130()[0]
    for k in (NINE.index(0), NINE.index(130)):
        assert count[k] == 0 and s1[k] == 0 and s2[k] == 0 and sd[k] == 0 and z[k] == 0 and p[k] == 0
    assert base[NINE.index(0)] == 0 and base[NINE.index(130)] == scores.astype(np.float64).sum()


def test_the_mirror_splits_by_first():
    scores, ptr, idx = case_130()
    base, count, s1, s2 = ref_130()
    a = pathway_ref(scores, ptr, idx, 7, 0, 1000)
    b = pathway_ref(scores, ptr, idx, 7, 1000, 3096)
    assert np.array_equal(a[0], base) and np.array_equal(a[1] + b[1], count)
    assert np.array_equal(a[2] + b[2], s1) and np.array_equal(a[3] + b[3], s2)       # exact: the scores are dyadic


def test_the_ordinary_case_has_no_comparison_within_rounding():
    base, count, s1, s2, close = ref_ordinary()
    print("ordinary scores, seed %d: %d comparisons within the summation bound; counts %s" % (ORDINARY_SEED, close, count))
    assert close == 0 and np.all((count > 0) & (count < 4096))


# --------------------------------------------------------------------------- host functions
def test_consolidate_gene_scores_reproduces_the_script():
    import phoenix_amd
    g = load_golden("g24_pathways")
    names, scores = phoenix_amd.consolidate_gene_scores(g["names"].tolist(), g["scores"])
    assert names == g["c_names"].tolist()
    assert scores.dtype == np.float64 and np.array_equal(scores, g["c_scores"])
    # the same from a tensor; a part that repeats a single name is averaged with it, a part that repeats in its entry is not
    names2, scores2 = phoenix_amd.consolidate_gene_scores(g["names"].tolist(), torch.from_numpy(g["scores"]))
    assert names2 == names and np.array_equal(scores2, scores)
    s = dict(zip(g["names"].tolist(), g["scores"].astype(np.float64).tolist()))
    got = dict(zip(names, scores.tolist()))
    assert got["ACE2"] == (s["ACE2"] + s["CSAG2 /// ACE2"]) / 2
    assert got["CES1"] == s["CES1 /// CES1 /// LOC100653057"] == got["LOC100653057"]
    assert names.index("ACE2") < names.index("C4A") < names.index("C4B_2")          # singles first, then the split entries
    assert not any("///" in n for n in names) and len(set(names)) == len(names)
    with pytest.raises(ValueError, match="consolidate_gene_scores"):
        phoenix_amd.consolidate_gene_scores(["a", "b"], [1.0])
    names, scores = phoenix_amd.consolidate_gene_scores(["b", " x /// b///x ", "a", "b"], [1.0, 4.0, 2.0, 3.0])
    assert names == ["b", "a", "x"] and scores.tolist() == [(1.0 + 3.0 + 4.0) / 3, 2.0, 4.0]


def test_read_pathways_reproduces_the_script(tmp_path):
    import phoenix_amd
    g = load_golden("g24_pathways")
    path = tmp_path / "go_bp_pathway_binary_wide.csv"
    path.write_text(str(g["table"]))
    for fp in (str(path), io.StringIO(str(g["table"]))):
        pw = phoenix_amd.read_pathways(fp, g["c_names"].tolist())
        assert isinstance(pw, phoenix_amd.Pathways) and pw._fields == ("names", "ptr", "idx", "kept")
        assert pw.names == g["p_names"].tolist()
        for key in ("ptr", "idx", "kept"):
            got = getattr(pw, key)
            assert got.dtype == g[key].dtype and np.array_equal(got, g[key]), key
    sizes = np.diff(pw.ptr)
    assert sizes.min() == 0 and sizes.max() == len(pw.kept) and len(pw.kept) < len(g["c_names"])
    with pytest.raises(ValueError, match="read_pathways"):
        phoenix_amd.read_pathways(io.StringIO("a,b\n1,0\n"), ["a"])
    with pytest.raises(ValueError, match="read_pathways"):
        phoenix_amd.read_pathways(io.StringIO(str(g["table"])), ["ACE2", "ACE2"])


def _result(base, count, s1, s2, n_perm, first=0, seed=0):
    import phoenix_amd
    return phoenix_amd.PermutationTest(torch.tensor(base, dtype=torch.float64), torch.tensor(count, dtype=torch.int64),
                                       torch.tensor(s1, dtype=torch.float64), torch.tensor(s2, dtype=torch.float64),
                                       n_perm, first, seed)


def test_write_permutation_table_byte_for_byte(tmp_path):
    import phoenix_amd
    # R = 4: mean = base + s1 / 4, var = (s2 - s1^2 / 4) / 3.  Pathways b and d tie at z = 1.5, c has sd = 0.
    res = _result(base=[1.0, 4.0, 2.5, 5.5, 0.125], count=[2, 0, 0, 1, 4], s1=[2.0, -6.0, 0.0, -6.0, 1.0],
                  s2=[13.0, 12.0, 0.0, 12.0, 0.296875], n_perm=4)
    z = res.z.tolist()
    assert z[1] == z[3] == 1.5 and z[2] == 0.0 and res.sd.tolist()[2] == 0.0
    expected = ('"pathway","phnx_z_score","mean_path_score","sd_path_score","phnx_p_val"\n'
                '"b",1.5,2.5,1,0\n'
                '"d, with a comma",1.5,4,1,0.25\n'
                '"c",0,2.5,0,0\n'
                '"a",-0.25,1.5,2,0.5\n'
                '"e",-2,0.375,0.125,1\n')
    names = ["a", "b", "c", "d, with a comma", "e"]
    buf = io.StringIO()
    assert phoenix_amd.write_permutation_table(buf, res, names) == 5
    assert buf.getvalue() == expected
    assert phoenix_amd.write_permutation_table(str(tmp_path / "permtest.csv"), res, names) == 5
    assert (tmp_path / "permtest.csv").read_text() == expected
    assert expected == table_ref(names, *stats_ref(*(x.numpy() for x in (res.base, res.count, res.s1, res.s2)), 4))
    with pytest.raises(ValueError, match="write_permutation_table"):
        phoenix_amd.write_permutation_table(io.StringIO(), res, names[:4])


def test_merge_adds_and_refuses():
    import phoenix_amd
    a = _result([1.0, 2.0], [3, 0], [0.5, -1.0], [2.0, 3.0], n_perm=10, first=0, seed=5)
    b = _result([1.0, 2.0], [4, 1], [1.5, -2.0], [1.0, 5.0], n_perm=6, first=10, seed=5)
    for m in (phoenix_amd.PermutationTest.merge(a, b), phoenix_amd.PermutationTest.merge(b, a)):
        assert (m.n_perm, m.first, m.seed) == (16, 0, 5)
        assert m.count.tolist() == [7, 1] and m.s1.tolist() == [2.0, -3.0] and m.s2.tolist() == [3.0, 8.0]
        assert m.base.tolist() == [1.0, 2.0] and m.p.tolist() == [7 / 16, 1 / 16]
        assert m.mean.tolist() == [1.0 + 2.0 / 16, 2.0 - 3.0 / 16]
    with pytest.raises(ValueError, match="seeds"):
        phoenix_amd.PermutationTest.merge(a, _result([1.0, 2.0], [4, 1], [1.5, -2.0], [1.0, 5.0], 6, first=10, seed=6))
    for first in (9, 0, 11, 4):                                     # overlapping, or with a gap
        with pytest.raises(ValueError, match="adjacent"):
            phoenix_amd.PermutationTest.merge(a, _result([1.0, 2.0], [4, 1], [1.5, -2.0], [1.0, 5.0], 6, first=first, seed=5))
    with pytest.raises(ValueError, match="same scores"):
        phoenix_amd.PermutationTest.merge(a, _result([1.0, 2.5], [4, 1], [1.5, -2.0], [1.0, 5.0], 6, first=10, seed=5))
    with pytest.raises(ValueError, match="at least 2"):
        _result([1.0], [0], [0.0], [0.0], n_perm=1).sd


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_pathway_permutations_workspace_bytes", "phx_pathway_permutations"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    assert mod.PATHWAYS_MAX_N == 16384 and mod.PATHWAYS_MAX_R == 2 ** 50
    import phoenix_amd
    for name in ("consolidate_gene_scores", "read_pathways", "pathway_permutation_test", "write_permutation_table", "Pathways",
                 "PermutationTest"):
        assert getattr(phoenix_amd, name) is getattr(phoenix_amd.analysis, name), name
    from phoenix_amd import build
    assert any(s.endswith("phx_pathways.hip") for s in build.sources())


def _call(lib, scores=0x1000, N=130, ptr=0x2000, idx=0x3000, P=9, nnz=411, seed=7, first=0, n_perm=500, base=0x4000,
          count=0x5000, s1=0x6000, s2=0x7000, ws=0x8000, ws_bytes=1 << 40):
    """phx_pathway_permutations with made-up device addresses: only calls that must return before touching the device"""
    return lib.phx_pathway_permutations(scores, N, ptr, idx, P, nnz, seed, first, n_perm, base, count, s1, s2, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    _, lib = _lib()
    for bad in (dict(N=0), dict(N=-1), dict(N=16385), dict(P=0), dict(P=-3), dict(nnz=-1), dict(n_perm=0), dict(n_perm=-5),
                dict(first=-1), dict(first=2 ** 50, n_perm=1), dict(first=2 ** 50 - 499), dict(n_perm=2 ** 50 + 1),
                dict(first=2 ** 62, n_perm=2 ** 62)):
        assert _call(lib, **bad) == BAD_ARG, bad
    for name in ("scores", "ptr", "idx", "base", "count", "s1", "s2"):
        assert _call(lib, **{name: None}) == BAD_ARG, name
    # every argument in order: the workspace is asked for next
    need = lib.phx_pathway_permutations_workspace_bytes(130, 9, 411, 500)
    assert need > 0
    for kw in (dict(), dict(N=1), dict(N=16384), dict(first=2 ** 50 - 500), dict(seed=2 ** 64 - 1), dict(idx=None, nnz=0),
               dict(n_perm=1)):
        assert _call(lib, ws=None, **kw) == WORKSPACE, kw
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(lib, ws_bytes=need, n_perm=512) == WORKSPACE             # more workgroups, more rows of partials


def test_workspace_bytes():
    _, lib = _lib()
    f = lib.phx_pathway_permutations_workspace_bytes
    assert f.restype is C.c_size_t
    for args in ((0, 9, 411, 500), (16385, 9, 411, 500), (130, 0, 411, 500), (130, 9, -1, 500), (130, 9, 411, 0),
                 (130, 9, 411, 2 ** 50 + 1)):
        assert f(*args) == 0, args
    # the members as 16-bit words and 24 bytes per workgroup and pathway, min(n_perm, 512) workgroups; N does not matter
    for P, nnz, R, G in ((9, 411, 3, 3), (9, 411, 500, 500), (9, 411, 10 ** 6, 512), (7000, 875000, 10 ** 5, 512), (1, 0, 1, 1)):
        exact = 2 * nnz + 24 * G * P
        assert exact <= f(130, P, nnz, R) <= exact + 4 * 256, (P, nnz, R)
        assert f(130, P, nnz, R) == f(16384, P, nnz, R) == f(1, P, nnz, R)
    assert f(130, 9, 411, 512) == f(130, 9, 411, 2 ** 50)


# --------------------------------------------------------------------------- the Python callers
def test_python_callers_refuse_bad_arguments_and_host_tensors():
    import phoenix_amd
    from phoenix_amd import engine
    scores, ptr, idx = case_130()
    pw = phoenix_amd.Pathways(["p%d" % k for k in range(len(NINE))], ptr, idx, np.arange(130))
    test = phoenix_amd.pathway_permutation_test
    for kw in (dict(n_perm=0), dict(n_perm=-1), dict(n_perm=2.5), dict(n_perm=True), dict(n_perm=None), dict(n_perm=1),
               dict(first=-1), dict(first=0.0), dict(first=2 ** 50), dict(first=2 ** 50 - 499), dict(seed=-1), dict(seed=2 ** 64),
               dict(seed=1.5), dict(seed=None)):
        with pytest.raises(ValueError, match="pathway_permutation_test"):
            test(scores, pw, **kw)
    bad_idx, dup_idx = idx.copy(), idx.copy()
    bad_idx[5] = 130
    dup_idx[ptr[5] + 1] = dup_idx[ptr[5]]
    neg_idx = idx.copy()
    neg_idx[0] = -1
    for bad in ((ptr, bad_idx), (ptr, neg_idx), (ptr, dup_idx), (ptr[:-1], idx), (ptr + 1, idx), (ptr[::-1].copy(), idx),
                (ptr[:1], idx[:0]), (ptr.astype(np.float64), idx), (ptr, idx.astype(np.float32))):
        with pytest.raises(ValueError, match="pathway_permutation_test"):
            test(scores, ("names",) + bad)
    for bad in (scores[:0], np.zeros(16385, np.float32), scores.reshape(13, 10), np.full(130, np.nan, np.float32),
                np.where(np.arange(130) == 7, np.inf, scores).astype(np.float32)):
        with pytest.raises(ValueError, match="pathway_permutation_test"):
            test(bad, pw) if bad.ndim != 1 or bad.shape[0] != 130 else test(bad, pw)
    with pytest.raises(RuntimeError, match="GPU"):
        test(scores, pw, device="cpu")
    # the engine call takes device tensors only, like the rest of the package
    s, p, i = torch.from_numpy(scores), torch.from_numpy(ptr), torch.from_numpy(idx)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        engine.pathway_permutations(s, p, i, 7, 0, 500)
    with pytest.raises(TypeError, match="tensor"):
        engine.pathway_permutations(scores, p, i, 7, 0, 500)
    for kw in (dict(seed=-1), dict(first=-1), dict(n_perm=0), dict(first=2 ** 50)):
        args = dict(seed=7, first=0, n_perm=500)
        args.update(kw)
        with pytest.raises(ValueError, match="pathway_permutations"):
            engine.pathway_permutations(s, p, i, **args)
