#!/usr/bin/env python3
"""Generate G24, the fixture of `consolidate_gene_scores` / `read_pathways` (and the input of the end-to-end permutation
test): the first 300 names of the reference's breast_cancer_data/clean_data/desmedt_gene_names_500.csv (a list of names;
it holds "A /// B /// C" entries), two of them edited so that a part repeats a single name ("CSAG2 /// CSAG3" becomes
"CSAG2 /// ACE2") and a part repeats inside one entry ("CES1 /// LOC100653057" becomes "CES1 /// CES1 /// LOC100653057";
the list's own "IGKV1-17 /// IGKV1-17" does that too), random scores, and a wide 0/1 pathway table of 12 pathways with a
repeated pathway row, a gene column that no name matches and an all-zero row.  The expected arrays are a plain-loop
restatement of create_permutation_test_files_aws.R:68-100 written out below; the package is not imported.

Runs only where the reference is mounted, on the CPU, and is never imported by a test.  Data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pathways.py

Keys of g24_pathways.npz:
    names [300] str, scores [300] float32      the entries and their influence scores
    c_names [C] str, c_scores [C] float64      R:68-84: the consolidated genes, in the script's order
    table                                      the text of the wide pathway table (header + 13 rows)
    p_names [12] str, ptr [13] int64, idx [nnz] int32, kept [K] int64
                                               R:90-100: the pathways, first row of a repeated one; the members as positions
                                               in the kept genes; the kept genes as indices into c_names
"""
import csv
import io
import os

import numpy as np

NAMES = "/root/reference/breast_cancer_data/clean_data/desmedt_gene_names_500.csv"
OUT = os.path.dirname(os.path.abspath(__file__))
EDITS = {"CSAG2 /// CSAG3": "CSAG2 /// ACE2", "CES1 /// LOC100653057": "CES1 /// CES1 /// LOC100653057"}


def consolidate(names, scores):
    """R:68-84, line by line"""
    single = []                                            # :68
    for n, s in zip(names, scores):
        if "///" not in n:
            single.append((n, s))
    multi = []                                             # :70-73: by = gene, then unique() over (gene, gene_split, influence)
    for n, s in zip(names, scores):
        if "///" in n:
            for part in n.split("///"):
                row = (n, part.strip(), s)
                if row not in multi:
                    multi.append(row)
    table = single + [(part, s) for _, part, s in multi]   # :75-79
    out_names, sums, counts = [], [], []                   # :84: mean by gene, groups in order of first appearance
    for n, s in table:
        if n in out_names:
            k = out_names.index(n)
            sums[k] += s
            counts[k] += 1
        else:
            out_names.append(n)
            sums.append(s)
            counts.append(1)
    return out_names, [a / c for a, c in zip(sums, counts)], counts


def main():
    with open(NAMES, newline="") as f:
        names = [row[0] for row in list(csv.reader(f))[1:301]]
    assert len(names) == 300 and all(k in names for k in EDITS)
    names = [EDITS.get(n, n) for n in names]
    assert "ACE2" in names and sum("///" in n for n in names) >= 10
    rng = np.random.default_rng(24)
    scores = rng.random(300).astype(np.float32)
    c_names, c_scores, counts = consolidate(names, [float(s) for s in scores])
    assert counts[c_names.index("ACE2")] == 2 and counts[c_names.index("CES1")] == 1 and len(set(c_names)) == len(c_names)
    assert counts[c_names.index("IGKV1-17")] == 1
    print("entries 300 -> genes %d, %d of them averaged" % (len(c_names), sum(c > 1 for c in counts)))

    # the table: two of every three consolidated genes are columns, in shuffled order, plus a column no name matches
    cols = [c_names[k] for k in rng.permutation(len(c_names)) if k % 3 != 1] + ["NOT_A_GENE"]
    cols.insert(5, cols.pop())                            # (somewhere in the middle)
    P = 12
    sizes = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 0, len(cols) - 1]
    rows = []
    for p in range(P):
        member = np.zeros(len(cols), np.int64)
        pick = [k for k in rng.permutation(len(cols)) if cols[k] != "NOT_A_GENE"][:sizes[p]]
        member[pick] = 1
        if p % 2:
            member[cols.index("NOT_A_GENE")] = 1
        rows.append(["PATH_%02d" % p] + member.tolist())
    again = ["PATH_03"] + (1 - np.array(rows[3][1:])).tolist()      # a second row of PATH_03: ignored
    rows.insert(7, again)
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n")
    w.writerow(["pathway"] + cols)
    w.writerows(rows)
    table = buf.getvalue()

    # R:90-100 on that text
    lines = list(csv.reader(io.StringIO(table)))
    header = lines[0]
    kept = [k for k, n in enumerate(c_names) if n in header[1:]]            # :90, in the order of the genes
    p_names, ptr, idx = [], [0], []
    for row in lines[1:]:
        if row[0] in p_names:
            continue                                                       # :18-19: [1, 1] of the product is the first row's
        p_names.append(row[0])
        for j, k in enumerate(kept):
            if int(row[header.index(c_names[k])]) == 1:
                idx.append(j)
        ptr.append(len(idx))
    got = np.diff(ptr).tolist()
    assert len(p_names) == P and got == sizes, (got, sizes)
    print("pathways %d, kept genes %d of %d, members %d" % (P, len(kept), len(c_names), len(idx)))
    np.savez_compressed(os.path.join(OUT, "g24_pathways.npz"), names=np.array(names), scores=scores, c_names=np.array(c_names),
                        c_scores=np.array(c_scores, np.float64), table=np.array(table), p_names=np.array(p_names),
                        ptr=np.array(ptr, np.int64), idx=np.array(idx, np.int32), kept=np.array(kept, np.int64))


if __name__ == "__main__":
    main()
