#!/usr/bin/env python3
"""Generate G21, the fixture of `effects_edges(orient=True)`: the reference's own `make_mask`
(extract_model_matrix_PHOENIX.py:29-37, lifted out of the script by AST like the effects-matrix statements of
make_golden_effects.py: the script loads checkpoints from hard-coded paths) run on a copy of the reference effects matrix
of a seeded dense reference ODENet.

Runs only where the reference is mounted, on the CPU, and is never imported by a test.  Data only.
Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edges.py

Keys of g21_edges.npz:
    p_*        the network (N = 37, H = 5, dense weights randn * 0.6 / sqrt(N), gene_multipliers = rand - 0.2)
    effects    float32 [N, N], the reference's `effects_mat` (regulator i -> target j)
    masked     float32 [N, N], the same after the reference's make_mask: of every pair the stronger direction only
"""
import ast
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)
import make_golden_effects as mge  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, H, SEED = 37, 5, 21


def reference_make_mask():
    src = open(os.path.join(mg.REF, "extract_model_matrix_PHOENIX.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "make_mask"]
    assert len(fn) == 1 and 29 <= fn[0].lineno <= 37
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "<reference extract_model_matrix_PHOENIX.py:make_mask>", "exec"), ns)
    return ns["make_mask"]


def abs_formula(p):
    """A of tests/test_effects_cpu.closed_form: the effects formula on absolute values, float64"""
    Ws, Wp, WaT = (np.abs(p[k].astype(np.float64)) for k in ("Ws", "Wp", "Wa"))
    WaT = WaT.T
    return np.maximum(p["g"].astype(np.float64), 0.0) * (Ws.T @ WaT[:H] + Wp.T @ WaT[H:])


def main():
    net = mg.make_net(N, H, seed=SEED, dense_std=0.6 / np.sqrt(N))
    with torch.no_grad():
        net.gene_multipliers.copy_(torch.rand(1, N) - 0.2)
    effects = mge.reference_effects(net)
    masked = effects.copy()
    reference_make_mask()(masked)
    # what the tests rely on, from the reference alone
    p = mg.params_np(net)
    assert effects.dtype == masked.dtype == np.float32 and effects.shape == masked.shape == (N, N)
    assert int((p["g"] <= 0).sum()) >= 2, p["g"]
    assert np.all(np.diag(masked) == 0)
    # no orientation is within reach of rounding: with b = (2H + 16) 2^-24 A (tests/test_effects_cpu.kernel_bound) both the
    # kernel's and the reference's entries lie within b of the exact ones, so a gap of 4 max(b_ij, b_ji) >= 2 (b_ij + b_ji)
    # between the magnitudes cannot be closed
    b = (2 * H + 16) * 2.0 ** -24 * abs_formula(p)
    gap = np.abs(np.abs(effects.astype(np.float64)) - np.abs(effects.astype(np.float64)).T)
    need = 4 * np.maximum(b, b.T)
    off = ~np.eye(N, dtype=bool)
    assert not np.any(gap[off] < need[off]), "seed %d: %d pairs too close, change the seed" % (SEED, int((gap[off] < need[off]).sum()))
    live = need[off] > 0
    print("multipliers <= 0: %d   edges kept: %d of %d   smallest gap / (4 x bound) = %.1f"
          % (int((p["g"] <= 0).sum()), int((masked != 0).sum()), N * N, float(np.min(gap[off][live] / need[off][live]))))
    mg.save("g21_edges", effects=effects, masked=masked, **mg.pfx(p, "p_"))


if __name__ == "__main__":
    main()
