#!/usr/bin/env python3
"""Generate G22, the fixture of `network_score` / `read_network`: the reference's own ranking and scoring of a matrix against
the shipped ChIP validation network, on a sub-network small enough for its Python lists.

  * the first 200 names of breast_cancer_data/clean_data/desmedt_gene_names_500.csv and the rows of validation_network.csv
    whose two genes are among them (self-edges included), as CSV texts and as index pairs;
  * a seeded float32 [200, 200] matrix, quantised so that ties abound: about 30 % exact zeros, two all-zero columns, both
    signs, and one positive whose magnitude is the global maximum;
  * for |matrix| and for |make_mask(matrix)| (`make_mask` of extract_model_matrix_PHOENIX.py:29-37, lifted by AST as
    make_golden_edges.py does): the list `get_link_list` (GRN_rnaode.py:43-181, lifted by AST) ranks -- off-diagonal
    entries, all regulators --, labelled and scored as COMPUTE_GRN_AUROC does in its lines 16-21 (the function itself
    stops at `np.int`, which the installed numpy no longer has), plus sklearn's average_precision_score, roc_curve
    (drop_intermediate=False) and precision_recall_curve on the same list.  The reference ranks importances, which are not
    negative; the magnitudes are what `network_score` ranks.

Runs only where the reference is mounted, on the CPU, and is never imported by a test.  Data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_netscore.py

Keys of g22_netscore.npz:
    names_csv, network_csv   the two files' texts (header row and the rows used), as read_network takes them
    regulator, target        int64 [E]: the network's index pairs, ascending (regulator, target), no duplicates
    matrix, masked           float32 [200, 200]: the matrix and the reference's make_mask of it
    for x in (plain, orient):
      x_auroc, x_ap          float64: roc_auc_score (COMPUTE_GRN_AUROC) and average_precision_score
      x_n_pos, x_n_neg       labels of each class in the ranked list
      x_roc_thr, x_roc_tp, x_roc_fp     roc_curve: thresholds (float32 values; the first, above everything, is dropped)
                             and tpr * P, fpr * Nn rounded to the integers they are
      x_pr_thr, x_pr_precision, x_pr_recall   precision_recall_curve (the final (1, 0) point is dropped)
"""
import ast
import io
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)
from make_golden_edges import reference_make_mask  # noqa: E402

import numpy as np  # noqa: E402
from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score, roc_curve  # noqa: E402

N, SEED = 200, 22
DATA = os.path.join(os.path.dirname(os.path.dirname(mg.REF)), "breast_cancer_data", "clean_data")


def reference_get_link_list():
    src = open(os.path.join(mg.REF, "GRN_rnaode.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_link_list"]
    assert len(fn) == 1 and fn[0].lineno == 43
    ns = {}
    exec("from numpy import *\nfrom operator import itemgetter", ns)      # the module's own imports (GRN_rnaode.py:5,7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SyntaxWarning)                     # `is not 'all'`
        exec(compile(ast.Module(body=fn, type_ignores=[]), "<reference GRN_rnaode.py:get_link_list>", "exec"), ns)
    return ns["get_link_list"]


def network():
    import csv
    with open(os.path.join(DATA, "desmedt_gene_names_500.csv"), newline="") as f:
        rows = list(csv.reader(f))
    header, names = rows[0], [r[0] for r in rows[1:N + 1]]
    assert len(names) == N == len(set(names))
    index = {n: k for k, n in enumerate(names)}
    with open(os.path.join(DATA, "validation_network.csv"), newline="") as f:
        rows = list(csv.reader(f))
    kept = [r for r in rows[1:] if r[0] in index and r[1] in index]
    names_csv = io.StringIO()
    csv.writer(names_csv, lineterminator="\n").writerows([header] + [[n] for n in names])
    network_csv = io.StringIO()
    csv.writer(network_csv, quoting=csv.QUOTE_ALL, lineterminator="\n").writerows([rows[0]] + kept)
    pairs = sorted({(index[a], index[b]) for a, b in kept})
    return names_csv.getvalue(), network_csv.getvalue(), np.array(pairs, np.int64)


def matrix(pairs):
    rng = np.random.default_rng(SEED)
    M = (rng.integers(-12, 13, size=(N, N)) / 16.0).astype(np.float32) * rng.choice(np.float32([0.25, 1.0, 1.5]), size=(N, N))
    M[rng.random((N, N)) < 0.27] = 0.0
    M[:, [17, 140]] = 0.0                                   # relu(g_j) = 0
    off = pairs[pairs[:, 0] != pairs[:, 1]]
    i, j = off[len(off) // 2]
    assert j not in (17, 140)
    M[i, j] = -3.0                                          # a positive at the global maximum, and the stronger direction
    return M.astype(np.float32)


def scored(get_link_list, VIM, pairs):
    link = get_link_list(VIM)
    edges = [vi[0] for vi in link]                          # GRN_rnaode.py:12-18
    scores = [vi[1] for vi in link]
    edges_true = [tuple(edge) for edge in pairs.tolist()]   # :19
    label = np.array([(edge in edges_true) for edge in edges], dtype=int)     # :20 (np.int is gone)
    out = {"auroc": roc_auc_score(label, scores), "ap": average_precision_score(label, scores),      # :21
           "n_pos": int(label.sum()), "n_neg": int(len(label) - label.sum())}
    fpr, tpr, thr = roc_curve(label, scores, drop_intermediate=False)
    out["roc_thr"] = np.asarray(thr[1:], np.float32)
    assert np.array_equal(out["roc_thr"].astype(np.float64), thr[1:])
    out["roc_tp"] = np.rint(tpr[1:] * out["n_pos"]).astype(np.int64)
    out["roc_fp"] = np.rint(fpr[1:] * out["n_neg"]).astype(np.int64)
    assert np.allclose(out["roc_tp"] / out["n_pos"], tpr[1:], rtol=0, atol=1e-12)
    assert np.allclose(out["roc_fp"] / out["n_neg"], fpr[1:], rtol=0, atol=1e-12)
    prec, rec, pthr = precision_recall_curve(label, scores)
    out["pr_thr"] = np.asarray(pthr, np.float32)
    out["pr_precision"], out["pr_recall"] = prec[:-1], rec[:-1]
    return out


def main():
    names_csv, network_csv, pairs = network()
    M = matrix(pairs)
    masked = M.copy()
    reference_make_mask()(masked)
    gll = reference_get_link_list()
    arrs = dict(names_csv=np.array(names_csv), network_csv=np.array(network_csv), regulator=pairs[:, 0], target=pairs[:, 1],
                matrix=M, masked=masked)
    for tag, X in (("plain", M), ("orient", masked)):
        res = scored(gll, np.abs(X), pairs)
        arrs.update({tag + "_" + k: v for k, v in res.items()})
        print("%s: AUROC %.6f  AP %.6f  positives %d  negatives %d  roc points %d" %
              (tag, res["auroc"], res["ap"], res["n_pos"], res["n_neg"], len(res["roc_thr"])))
    # what the tests rely on
    off = pairs[pairs[:, 0] != pairs[:, 1]]
    assert arrs["plain_n_pos"] == len(off) == arrs["orient_n_pos"] and arrs["plain_n_pos"] + arrs["plain_n_neg"] == N * N - N
    assert np.abs(M).max() == 3.0 and (np.abs(M) == 3.0).sum() == 1 and (np.abs(masked) == 3.0).sum() == 1
    print("edges %d (self-edges %d, regulators %d)  zeros %.1f %%  distinct magnitudes %d" %
          (len(pairs), len(pairs) - len(off), len(set(pairs[:, 0].tolist())), 100 * float((M == 0).mean()),
           len(np.unique(np.abs(M)))))
    mg.save("g22_netscore", **arrs)


if __name__ == "__main__":
    main()
