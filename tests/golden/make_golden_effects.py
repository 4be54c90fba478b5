#!/usr/bin/env python3
"""Generate G20, the fixture of `effects_matrix` and `jacobian_matrix`: the reference's own effects-matrix statements
(extract_model_matrix_PHOENIX.py:46-58, lifted out of the script by AST: the file itself loads checkpoints from hard-coded
paths and imports a module the reference does not ship) run on the submodules of a seeded reference ODENet, and
torch.autograd.functional.jacobian of the reference's `forward` at three expression states, in float64 and in float32.

Like make_golden_backprop.py it runs only where the reference is mounted, on the CPU, and is never imported by a test.
Data only.  Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_effects.py

Keys of g20_effects.npz:
    p_*        the network (N = 37, H = 5, dense weights randn * 0.6 / sqrt(N), gene_multipliers = rand - 0.2)
    effects    float32 [N, N], the reference's `effects_mat` (regulator i -> target j)
    y          float32 [3, N] states in [-0.2, 1.2]; y[1, 5] = 0.5 exactly
    jac64      float64 [3, N, N], jac64[b, i, j] = d forward_j / d y_i at y[b], network and state in float64
    jac32      float32 [3, N, N], the same in float32
"""
import ast
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, H, B, SEED = 37, 5, 3, 20
FIRST, LAST = 46, 58      # the statements between the checkpoint loads and the CSV dump


def reference_effects(net):
    """runs the script's assignment statements of lines 46-58 on this network's submodules"""
    src = open(os.path.join(mg.REF, "extract_model_matrix_PHOENIX.py")).read()
    body = [n for n in ast.parse(src).body if isinstance(n, ast.Assign) and FIRST <= n.lineno <= LAST]
    assert len(body) == 10 and body[-1].targets[0].id == "effects_mat", [ast.dump(n.targets[0]) for n in body]
    ns = {"np": np, "torch": torch, "sums_model": net.net_sums, "prods_model": net.net_prods,
          "alpha_comb": net.net_alpha_combine, "gene_mult": net.gene_multipliers}
    exec(compile(ast.Module(body=body, type_ignores=[]), "<reference extract_model_matrix_PHOENIX.py:46-58>", "exec"), ns)
    return ns["effects_mat"]


def jacobians(net, y):
    """[B, N, N] with [b, i, j] = d forward_j / d y_i at y[b] (autograd returns [1, output j, input i]: gene_multipliers
    is [1, N])"""
    return torch.stack([torch.autograd.functional.jacobian(lambda v: net.forward(None, v), yb).reshape(N, N).t()
                        for yb in y])


def main():
    net = mg.make_net(N, H, seed=SEED, dense_std=0.6 / np.sqrt(N))
    with torch.no_grad():
        net.gene_multipliers.copy_(torch.rand(1, N) - 0.2)
    y = torch.rand(B, N) * 1.4 - 0.2
    y[1, 5] = 0.5
    effects = reference_effects(net)
    jac32 = jacobians(net, y)
    jac64 = jacobians(copy.deepcopy(net).double(), y.double())
    # what the tests rely on, from the reference alone
    g = net.gene_multipliers.detach().numpy().reshape(-1)
    assert effects.dtype == np.float32 and effects.shape == (N, N)
    assert int((g <= 0).sum()) >= 2, g
    assert int((y == 0.5).sum()) == 1 and bool((y < 0.5).any()) and bool((y > 0.5).any())
    assert bool((y >= -0.2).all()) and bool((y <= 1.2).all())
    assert jac64.dtype == torch.float64 and jac32.dtype == torch.float32 and jac64.shape == (B, N, N)
    print("multipliers <= 0: %d   max |jac32 - jac64| / max |jac64| = %.3e"
          % (int((g <= 0).sum()), float((jac32.double() - jac64).abs().max() / jac64.abs().max())))
    mg.save("g20_effects", effects=effects, y=y.numpy(), jac64=jac64.numpy(), jac32=jac32.numpy(),
            **mg.pfx(mg.params_np(net), "p_"))


if __name__ == "__main__":
    main()
