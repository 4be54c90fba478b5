#!/usr/bin/env python3
"""Times phoenix_amd.validation() against the loop it replaces (one odeint call per validation item, the reference's
train_insilico.py:77-106 on this package's odeint) on a synthetic validation set of breast-cancer scale.

    python tools/validation_time.py [--genes 11165] [--hidden 40] [--items 16] [--rows 7] [--method dopri5] [--reps 15]

Every item is `rows` states over rows + 1 times (a trajectory-type item; --rows 1 is the `single` type); every third item
misses its last time point.  Warm-up, then `reps` timed runs of each form with the device drained before and after each
run; prints median and min..max of both, the launch counts (ceil(K / calls per launch) per group against K) and the
largest difference of the two losses, one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phoenix_amd  # noqa: E402
from phoenix_amd import _lib  # noqa: E402


class Handler:
    """what validation() reads of a DataHandler"""

    def __init__(self, data, t, target):
        self.val_data, self.val_t, self.val_target, self.n_val = data, t, target, data.shape[0]

    def get_validation_set(self):
        return self.val_data, self.val_t, self.val_target, self.n_val


def loop_validation(net, h, method):
    data, t, target_full, n_val = h.get_validation_set()
    with torch.no_grad():
        predictions, targets = [], []
        for time_, batch_point, target_point in zip(t, data, target_full):
            idx = [i for i in range(len(time_)) if not torch.isnan(time_[i])]
            time_ = time_[idx]
            idx.pop()
            predictions.append(phoenix_amd.odeint(net, batch_point[idx], time_, method=method)[1])
            targets.append(target_point[idx])
        return torch.mean((torch.cat(predictions) - torch.cat(targets)) ** 2)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        out.item()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out.item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=11165)
    ap.add_argument("--hidden", type=int, default=40)
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--rows", type=int, default=7)
    ap.add_argument("--method", default="dopri5")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    N, K, R = a.genes, a.items, a.rows
    net = phoenix_amd.ODENet(dev, N, neurons=a.hidden)
    with torch.no_grad():
        for p in (net.net_sums.linear_out.weight, net.net_prods.linear_out.weight, net.net_alpha_combine.linear_out.weight):
            p.normal_(0.0, 0.6 / math.sqrt(N))
    data = torch.rand(K, R, 1, N, device=dev)
    target = torch.rand(K, R, 1, N, device=dev)
    t = torch.cumsum(0.05 + 0.1 * torch.rand(K, R + 1, dtype=torch.float64), 1).to(dev)
    if R > 1:
        t[::3, -1] = float("nan")
    h = Handler(data, t, target)
    lib, m = _lib.load(), _lib.METHODS[a.method]
    launches = {}
    for rows in sorted({R, R - 1} if R > 1 else {R}):
        k = int(sum(1 for i in range(K) if (R - 1 if (R > 1 and i % 3 == 0) else R) == rows))
        if k:
            launches[rows] = {"calls": k, "launches": lib.phx_debug_calls_grids_launches(N, a.hidden, rows * k, 2, k, m) if k > 1 else 1,
                              "kernel": lib.phx_debug_calls_grids_kernel_m(N, a.hidden, rows * k, 2, k, m)}
    batched = timed(lambda: phoenix_amd.validation(net, h, a.method, False)[0], a.reps)
    loop = timed(lambda: loop_validation(net, h, a.method), a.reps)
    print(json.dumps({"genes": N, "hidden": a.hidden, "items": K, "rows": R, "method": a.method, "reps": a.reps,
                      "validation_ms": {"median": batched[0], "min": batched[1], "max": batched[2]},
                      "loop_ms": {"median": loop[0], "min": loop[1], "max": loop[2]},
                      "groups": launches, "loss_rel_diff": abs(batched[3] - loop[3]) / abs(loop[3])}))


if __name__ == "__main__":
    main()
