#!/usr/bin/env python3
"""Generate G23, the fixture of `effects_neighbors` / `write_link_list`: the reference's own ranked link list
(`get_link_list`, GRN_rnaode.py:43-181, lifted by AST as make_golden_netscore.py does) of G21's effects matrix -- the network
and the `effects` / `masked` matrices of g21_edges.npz (N = 37, H = 5, two columns with g <= 0) -- with gene names g0 .. g36,
once with every gene a candidate regulator and once with the candidates [i for i in range(37) if i % 3 != 0].  The
reference ranks importances, which are not negative: it is run on |effects| and on |masked|.  Its list ends in a randomly
permuted tail of zero scores, which is cut off.

Runs only where the reference is mounted, on the CPU, and is never imported by a test.  Data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_neighbors.py

Keys of g23_neighbors.npz:
    candidates                 int64: the restricted candidate regulators
    for x in (plain, masked), c in (all, cand):
      x_c_regulator, x_c_target   int64 [E]: the ranked links with a non-zero score, in the reference's order
      x_c_score                   float32 [E]: their scores (|matrix entry|)
      x_c_text                    the file the reference writes with file_name= and maxcount=40
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)
from make_golden_edges import abs_formula  # noqa: E402
from make_golden_netscore import reference_get_link_list  # noqa: E402

import numpy as np  # noqa: E402

MAXCOUNT = 40


def ranked(gll, VIM, names, regulators):
    link = gll(VIM, gene_names=names, regulators=regulators)
    idx = {n: k for k, n in enumerate(names)}
    reg = np.array([idx[e[0][0]] for e in link], np.int64)
    tgt = np.array([idx[e[0][1]] for e in link], np.int64)
    score = np.array([e[1] for e in link], np.float32)
    assert np.array_equal(score, VIM[reg, tgt]) and np.all(np.diff(score.astype(np.float64)) <= 0)
    live = score != 0
    n = int(live.sum())
    assert np.all(live[:n]) and not np.any(live[n:])       # the zero scores are the tail
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "links.txt")
        gll(VIM, gene_names=names, regulators=regulators, maxcount=MAXCOUNT, file_name=path)
        text = open(path).read()
    assert n > MAXCOUNT and text.count("\n") == MAXCOUNT
    return reg[:n], tgt[:n], score[:n], text


def rank_gap(M, b, candidates):
    """the smallest gap between consecutive ranked magnitudes of a row or a column (over the live entries off the diagonal
    with a candidate regulator) relative to the sum of the two entries' rounding bounds"""
    N = M.shape[0]
    ok = (M != 0) & ~np.eye(N, dtype=bool)
    ok[[i for i in range(N) if i not in candidates], :] = False
    mag = np.abs(M.astype(np.float64))
    worst = np.inf
    for lines in (ok, ok.T):
        m2, b2 = (mag, b) if lines is ok else (mag.T, b.T)
        for n in range(N):
            sel = np.nonzero(lines[n])[0]
            order = sel[np.argsort(-m2[n, sel], kind="stable")]
            if len(order) > 1:
                gap = m2[n, order[:-1]] - m2[n, order[1:]]
                worst = min(worst, float(np.min(gap / (b2[n, order[:-1]] + b2[n, order[1:]]))))
    return worst


def main():
    g = np.load(os.path.join(mg.OUT, "g21_edges.npz"))
    p = {k[2:]: g[k] for k in g.files if k.startswith("p_")}
    effects, masked = g["effects"], g["masked"]
    H, N = p["Ws"].shape
    assert (N, H) == (37, 5)
    names = ["g%d" % i for i in range(N)]
    candidates = [i for i in range(N) if i % 3 != 0]
    gll = reference_get_link_list()
    # rounding cannot swap a rank: with b = (2H + 16) 2^-24 A (tests/test_effects_cpu.kernel_bound) the kernel's and the
    # reference's entries lie within b of the exact ones, so magnitudes further apart than 2 (b + b') keep their order
    b = (2 * H + 16) * 2.0 ** -24 * abs_formula(p)
    arrs = {"candidates": np.array(candidates, np.int64)}
    for tag, X in (("plain", effects), ("masked", masked)):
        for ctag, cand in (("all", list(range(N))), ("cand", candidates)):
            ratio = rank_gap(X, b, cand)
            assert ratio > 2.0, "%s %s: consecutive ranks within reach of rounding (ratio %.2f), change the seed of G21" % (tag, ctag, ratio)
            reg, tgt, score, text = ranked(gll, np.abs(X), names, "all" if ctag == "all" else [names[i] for i in cand])
            assert set(reg.tolist()) <= set(cand) and np.all(reg != tgt)
            assert len(score) == int(((X != 0) & ~np.eye(N, dtype=bool))[cand].sum())
            print("%-6s %-4s links %4d   smallest rank gap / (b + b') = %.1f" % (tag, ctag, len(score), ratio))
            arrs.update({"%s_%s_regulator" % (tag, ctag): reg, "%s_%s_target" % (tag, ctag): tgt,
                         "%s_%s_score" % (tag, ctag): score, "%s_%s_text" % (tag, ctag): np.array(text)})
    mg.save("g23_neighbors", **arrs)


if __name__ == "__main__":
    main()
