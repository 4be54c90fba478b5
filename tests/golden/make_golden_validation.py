#!/usr/bin/env python3
"""Generate G19, the fixture of `validation` and `get_true_val_set_r2`: the reference's own two functions
(train_insilico.py:77-106 and :51-61, cut out of the script as make_goldens.py cuts `training_step`) on the reference's own
ODENet, DataHandler and odeint, over tests/golden/g9_data.csv (10 genes, 7 trajectories, three of which miss their last
time points).

Like make_golden_backprop.py it runs only where the reference is mounted, on the CPU, and is never imported by a test.
Data only.  Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_validation.py

Keys of g19_validation.npz (case in traj / single):
    p_*                          the network (make_goldens.make_net(10, 6, seed 19, dense))
    <case>/seed, val_split       numpy seed in front of DataHandler.fromcsv, and its validation share
    <case>/val_t                 the validation set's times (traj: holds NaN), to check that the split was reproduced
    <case>/<method>/loss, n_val  validation(odenet, handler, method, False)
    <case>/<method>/r2, mse      get_true_val_set_r2(odenet, handler, method, <batch type>)
"""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (sets the reference path; its generators run under __main__ only)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torchdiffeq import odeint  # noqa: E402  (reference)

CASES = {"traj": ("trajectory", 0.45), "single": ("single", 0.3)}
METHODS = ("dopri5", "rk4")


def reference_functions():
    fns = {}
    for name in ("my_r_squared", "get_true_val_set_r2", "validation"):
        fns[name] = mg.load_reference_function(name)
    for f in fns.values():            # the functions find each other and the reference's odeint as the script's globals
        f.__globals__.update(fns)
        f.__globals__["odeint"] = odeint
    return fns


def handler(batch_type, val_split, want_nan):
    from datahandler import DataHandler as RefDataHandler     # reference
    csv_path = os.path.join(mg.OUT, "g9_data.csv")
    for seed in range(40, 240):
        with contextlib.redirect_stdout(io.StringIO()):
            np.random.seed(seed)
            h = RefDataHandler.fromcsv(csv_path, "cpu", val_split, normalize=False, batch_type=batch_type, noise=0.0)
        vt = h.get_validation_set()[1]
        if bool(torch.isnan(vt).any()) == want_nan:
            return h, seed
    raise AssertionError("no split of the wanted kind")


def main():
    fns = reference_functions()
    net = mg.make_net(10, 6, seed=19, dense_std=0.3)
    out = mg.pfx(mg.params_np(net), "p_")
    for case, (batch_type, val_split) in CASES.items():
        h, seed = handler(batch_type, val_split, want_nan=batch_type == "trajectory")
        out[case + "/seed"], out[case + "/val_split"] = np.int64(seed), np.float64(val_split)
        out[case + "/val_t"] = h.get_validation_set()[1].numpy()
        for method in METHODS:
            loss, n_val = fns["validation"](net, h, method, False)
            r2, mse = fns["get_true_val_set_r2"](net, h, method, batch_type)
            key = "%s/%s/" % (case, method)
            out[key + "loss"], out[key + "n_val"] = np.float64(loss.item()), np.int64(n_val)
            out[key + "r2"], out[key + "mse"] = np.float64(r2.item()), np.float64(mse.item())
            print(key, loss.item(), n_val, r2.item(), mse.item())
    mg.save("g19_validation", **out)


if __name__ == "__main__":
    main()
