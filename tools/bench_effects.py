#!/usr/bin/env python3
"""Effects matrix and state Jacobian, the kernel against the torch formulation (run on the MI355X):
    python tools/bench_effects.py [--shapes 11165x40,14691x200] [--B 60] [--repeats 10] [--out profiles/effects_matrix.json]
Per shape (N, H): PHX_EFFECTS (time, achieved write bandwidth: the mode moves N^2 * 4 bytes for about 4 N^2 H flops, so
the HBM write rate is the figure to judge it by) against two torch matmuls and a scale; PHX_JAC_MEAN_ABS over B states
(time, fraction of the 157.3 TFLOP/s fp32 matrix peak over 2 N^2 H (B + 1) flops) against a per-state torch loop; and the
largest difference between the two formulations' results.  Warm-up, HIP events, median of the repeats.  Reads nothing
outside the tree; writes one JSON file."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phoenix_amd as pa                                           # noqa: E402
from phoenix_amd import _lib, engine                               # noqa: E402
from phoenix_amd.odenet import params_of                           # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, the device's specified peak
FP32_PEAK = 157.3e12    # flop/s, fp32 matrix (= vector) peak


def timed(fn, repeats, warmup=2):
    """milliseconds of every repeat of fn(), by device events around it"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def torch_effects(p, out):
    H = p.H
    torch.matmul(p.Ws.t(), p.WaT[:H], out=out)
    out.addmm_(p.Wp.t(), p.WaT[H:])
    return out.mul_(torch.relu(p.g))


def torch_mean_abs(p, y, ph, acc, tmp):
    """per state: Q_b by one matmul, the combination by elementwise passes over the [N, N] buffers"""
    H = p.H
    r = torch.relu(p.g)
    s = y - 0.5
    da = 1 / (1 + s.abs()) ** 2
    dl = torch.where(s < 0, 1 / (1 + s.abs()), 1 / ((1 + s) * (1 + 2 * s)))
    S = p.Ws.t() @ p.WaT[:H]
    acc.zero_()
    for b in range(y.shape[0]):
        torch.matmul((p.Wp * ph[b][:, None]).t(), p.WaT[H:], out=tmp)
        tmp.mul_(dl[b][:, None]).addcmul_(S, da[b][:, None])
        tmp.diagonal().sub_(1.0)
        acc.add_(tmp.mul_(r).abs_())
    return acc.div_(y.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11165x40,14691x200")
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_matrix.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_effects.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))                            # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "B": a.B,
           "library_sha256": hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest(), "shapes": []}
    for shape in a.shapes.split(","):
        N, H = (int(v) for v in shape.split("x"))
        B = a.B
        torch.manual_seed(0)
        net = pa.ODENet(dev, N, neurons=H)
        with torch.no_grad():                                      # dense, trained-like weights
            for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
                lin.weight.normal_(0.0, 0.6 / np.sqrt(N))
            net.gene_multipliers.sub_(0.2)
        p = engine.params_cached(*params_of(net))
        y = torch.rand((B, N), device=dev) * 1.4 - 0.2
        s = y - 0.5
        ph = torch.exp(torch.addmm(p.bp, torch.log1p(s / (1 + s.abs())), p.Wp.t()))
        out = torch.empty((N, N), device=dev)
        ref, tmp = torch.empty((N, N), device=dev), torch.empty((N, N), device=dev)
        row = {"N": N, "H": H, "B": B, "matrix_bytes": N * N * 4}

        engine.effects_matrix(p, "effects", out=out)
        torch_effects(p, ref)
        row["effects_max_abs_diff_over_max_abs"] = float((out - ref).abs().max() / ref.abs().max())
        t_k = timed(lambda: engine.effects_matrix(p, "effects", out=out), a.repeats, warmup=3)
        t_t = timed(lambda: torch_effects(p, ref), a.repeats, warmup=3)
        t_fill = timed(lambda: out.fill_(1.0), a.repeats, warmup=3)    # what this device writes when it only writes
        bw = N * N * 4 / (med(t_k) * 1e-3)
        row["effects"] = {"kernel_ms": med(t_k), "torch_ms": med(t_t), "torch_over_kernel": med(t_t) / med(t_k),
                          "write_bytes_per_s": bw, "fraction_of_hbm_peak": bw / HBM_PEAK, "fill_same_bytes_ms": med(t_fill),
                          "kernel_over_fill": med(t_k) / med(t_fill), "flops": 4.0 * N * N * H,
                          "flop_per_s": 4.0 * N * N * H / (med(t_k) * 1e-3), "kernel_all_ms": t_k}

        engine.effects_matrix(p, "mean_abs", y=y, ph=ph, out=out)
        torch_mean_abs(p, y, ph, ref, tmp)
        row["mean_abs_max_abs_diff_over_max_abs"] = float((out - ref).abs().max() / ref.abs().max())
        t_k = timed(lambda: engine.effects_matrix(p, "mean_abs", y=y, ph=ph, out=out), a.repeats, warmup=2)
        t_a = timed(lambda: pa.jacobian_matrix(net, y, out=out), a.repeats, warmup=2)
        t_t = timed(lambda: torch_mean_abs(p, y, ph, ref, tmp), max(3, a.repeats // 3), warmup=1)
        flops = 2.0 * N * N * H * (B + 1)
        row["jac_mean_abs"] = {"kernel_ms": med(t_k), "jacobian_matrix_ms": med(t_a), "torch_ms": med(t_t),
                               "torch_over_kernel": med(t_t) / med(t_k), "flops": flops,
                               "flop_per_s": flops / (med(t_k) * 1e-3),
                               "fraction_of_fp32_peak": flops / (med(t_k) * 1e-3) / FP32_PEAK, "kernel_all_ms": t_k}
        res["shapes"].append(row)
        print("N=%d H=%d: effects %.3f ms = %.2f TB/s written (%.0f %% of 8 TB/s; fill %.3f ms; torch %.3f ms, %.2fx); "
              "mean |J| over %d states %.2f ms = %.1f TFLOP/s (%.0f %% of 157.3; torch %.1f ms, %.2fx)"
              % (N, H, row["effects"]["kernel_ms"], bw / 1e12, 100 * bw / HBM_PEAK, med(t_fill), row["effects"]["torch_ms"],
                 row["effects"]["torch_over_kernel"], B, med(t_k), flops / (med(t_k) * 1e-3) / 1e12,
                 100 * row["jac_mean_abs"]["fraction_of_fp32_peak"], med(t_t), row["jac_mean_abs"]["torch_over_kernel"]))
        del out, ref, tmp, net, p
        engine.forget_params()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["shapes"]))


if __name__ == "__main__":
    main()
