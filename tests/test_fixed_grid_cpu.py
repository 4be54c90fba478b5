"""CPU-only checks of the fixed-grid truth tests (tests/test_fixed_grid_truth_gpu.py): the launch geometries that file is
there for, held to the planner at the 256 CUs of an MI355X without a device; the condition on the inputs of tests/g26.py
(every figure of the float32 references at most TOL_FIXED / 2 from the float64 truth); and the float64 arbiter of
tests/g26.py against golden G26, the reference's own odeint_adjoint in float64.

GEOMETRY: name -> ((N, H, B, control, env), forward plan, backward plan) with T = 5 and rk4 (euler and midpoint plan
alike, asserted below).  The forward kernel is 1 (k1_solve_fwd); the backward kernel is the first that plans the batch,
2 (k1_solve_adj2) before 1 (k1_solve_adj); a plan of None is the VALU kernel's case (k_solve_fwd / k_solve_adj).  control is what the
caller asks for with a 1-D t: "shared" (the default: one batch group) or options={"batch_control": "per_trajectory"}.  A
step size plans per trajectory whatever the caller asked, so the GPU file runs a step size on the per_trajectory rows
only: on a shared row it would run the geometry of the per_trajectory row of the same shape.
Template instantiations by plan: k1_solve_fwd<HT, 64 NW[, CH if HC = 2]>; k1_solve_adj2 in its 8-wave (NW = 8) and 4-wave
form; k1_solve_adj<HT[, CH]> in workgroups of NW = 1, 2 or 4 waves."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import g26

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_table as pt  # noqa: E402

ODEINT, ADJOINT = 2, 3
T = len(g26.T5)
LDS_BUDGET = 163840 - 1024   # csrc/phx_host.hpp
CPU_MAX = 3551 * 49 * 150    # N x H x B up to which a case's arbiters run here in a few seconds
WANT = ("HT", "HC", "NW", "TPW", "NB", "G", "TG", "ntg", "nblk")

GEOMETRY = {
    "h7_b1": ((45, 7, 1, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2)),
    "h7_b61": ((45, 7, 61, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h7_b64": ((45, 7, 64, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h7_b100_s": ((45, 7, 100, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=7, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2)),
    "h7_b100_p": ((45, 7, 100, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=2, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=2, ntg=4, nblk=2)),
    "h7_b150_s": ((45, 7, 150, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=2, NB=1, G=2, TG=1, ntg=10, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2)),
    "h7_b300_s": ((45, 7, 300, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=4, NB=1, G=2, TG=1, ntg=19, nblk=2),
        None),
    "n350_b1530_s": ((350, 7, 1530, "shared", {}),      # 96 tiles in one batch group: no MFMA kernel either way
        None,
        None),
    "h7_b300_p": ((45, 7, 300, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=5, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=5, ntg=4, nblk=2)),
    "n1100_b1": ((1100, 7, 1, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=1, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=1, nblk=35)),
    "n1100_b61_s": ((1100, 7, 61, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35)),
    "n1100_b64_s": ((1100, 7, 64, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35)),
    "n1100_b64_p": ((1100, 7, 64, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=1, TPW=1, NB=1, G=35, TG=4, ntg=1, nblk=35)),
    "n1100_b61_p": ((1100, 7, 61, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=4, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=1, TPW=1, NB=1, G=35, TG=4, ntg=1, nblk=35)),
    "n1100_b100_s": ((1100, 7, 100, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=1, G=35, TG=1, ntg=7, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=2, NB=1, G=35, TG=1, ntg=7, nblk=35)),
    "n1100_b150_s": ((1100, 7, 150, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=2, NB=1, G=35, TG=1, ntg=10, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=4, NB=1, G=35, TG=1, ntg=10, nblk=35)),
    "n1100_b150_p": ((1100, 7, 150, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=3, ntg=4, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=2, TPW=1, NB=1, G=35, TG=5, ntg=2, nblk=35)),
    "n3551_h7_p": ((3551, 7, 150, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=1, G=111, TG=2, ntg=8, nblk=111),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111)),
    "n1100_b1530": ((1100, 7, 1530, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=2, G=18, TG=12, ntg=8, nblk=35),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=4, G=9, TG=24, ntg=4, nblk=35)),
    "n350_b1530": ((350, 7, 1530, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=1, G=11, TG=12, ntg=8, nblk=11),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=2, G=6, TG=24, ntg=4, nblk=11)),
    "n2000_h7": ((2000, 7, 520, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=3, G=21, TG=9, ntg=4, nblk=63),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=3, G=21, TG=9, ntg=4, nblk=63)),
    "n700_b4096": ((700, 7, 4096, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=3, G=8, TG=32, ntg=8, nblk=22),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=6, G=4, TG=64, ntg=4, nblk=22)),
    "n700_b4093": ((700, 7, 4093, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=8, TPW=1, NB=3, G=8, TG=32, ntg=8, nblk=22),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=6, G=4, TG=64, ntg=4, nblk=22)),
    "h48_b61": ((45, 48, 61, "shared", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h49_b1": ((45, 49, 1, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2)),
    "h49_b17": ((45, 49, 17, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2)),
    "h49_b37_s": ((45, 49, 37, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=3, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=3, nblk=2)),
    "h49_b37_p": ((45, 49, 37, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=3, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=2, ntg=2, nblk=2)),
    "h49_b61": ((45, 49, 61, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h49_b64": ((45, 49, 64, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h49_b100_s": ((45, 49, 100, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=7, nblk=2)),
    "h49_b150_s": ((45, 49, 150, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2)),
    "n3551_h49_b150": ((3551, 49, 150, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=1, NB=3, G=37, TG=5, ntg=2, nblk=111)),
    "n3551_h49_b200": ((3551, 49, 200, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=2, G=56, TG=4, ntg=4, nblk=111),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=2, G=56, TG=4, ntg=4, nblk=111)),
    "n2000_h49": ((2000, 49, 520, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=3, G=21, TG=9, ntg=4, nblk=63),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=3, G=21, TG=9, ntg=4, nblk=63)),
    "n2000_h100": ((2000, 100, 520, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=2, NB=2, G=32, TG=5, ntg=8, nblk=63),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=4, NB=2, G=32, TG=5, ntg=8, nblk=63)),
    "h128_b61": ((45, 128, 61, "shared", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h129_b1": ((45, 129, 1, "shared", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2)),
    "h129_b64_s": ((45, 129, 64, "shared", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h129_b61_p": ((45, 129, 61, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=1, TPW=1, NB=1, G=2, TG=4, ntg=1, nblk=2)),
    "h129_b64_p": ((45, 129, 64, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=1, TPW=1, NB=1, G=2, TG=4, ntg=1, nblk=2)),
    "h129_b100_s": ((45, 129, 100, "shared", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2)),
    "h129_b100_p": ((45, 129, 100, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=2, ntg=4, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=1, TPW=1, NB=1, G=2, TG=7, ntg=1, nblk=2)),
    "h129_b150_s": ((45, 129, 150, "shared", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2)),
    "h224_b61": ((45, 224, 61, "shared", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "n700_h129": ((700, 129, 200, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=22, TG=4, ntg=4, nblk=22),
        dict(kernel=1, HT=7, HC=2, NW=2, TPW=1, NB=1, G=22, TG=7, ntg=2, nblk=22)),
    "n3551_h129": ((3551, 129, 150, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111)),
    "h226_b1": ((45, 226, 1, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=1, nblk=2)),
    "h226_b64_s": ((45, 226, 64, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h226_b61_s": ((45, 226, 61, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "h226_b100_s": ((45, 226, 100, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=7, nblk=2)),
    "h226_b150_s": ((45, 226, 150, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=4, NB=1, G=2, TG=1, ntg=10, nblk=2)),
    "h256_b61": ((45, 256, 61, "shared", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "n3551_h226": ((3551, 226, 150, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111),
        dict(kernel=1, HT=8, HC=2, NW=4, TPW=1, NB=2, G=56, TG=3, ntg=4, nblk=111)),
    "v2np2_h7": ((45, 7, 61, "shared", {"PHX_ADJ": "v2", "PHX_ADJ2_NP": "2"}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=4, TPW=2, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "v2np4_h49": ((45, 49, 61, "shared", {"PHX_ADJ": "v2", "PHX_ADJ2_NP": "4"}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    "v1_h49": ((45, 49, 61, "shared", {"PHX_ADJ": "v1"}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=4, nblk=2)),
    # per-sample grids (t [B, 2-D]): B <= 20, the arbiter solves the rows one by one
    "ps_h7": ((45, 7, 19, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2),
        dict(kernel=2, HT=3, HC=1, NW=8, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2)),
    "ps_h49": ((45, 49, 19, "per_trajectory", {}),
        dict(kernel=1, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2),
        dict(kernel=2, HT=8, HC=1, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2)),
    "ps_n1100": ((1100, 7, 19, "per_trajectory", {}),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=2, nblk=35),
        dict(kernel=1, HT=3, HC=1, NW=4, TPW=1, NB=1, G=35, TG=1, ntg=2, nblk=35)),
    "ps_h129": ((45, 129, 19, "per_trajectory", {}),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2),
        dict(kernel=1, HT=7, HC=2, NW=4, TPW=1, NB=1, G=2, TG=1, ntg=2, nblk=2)),
}
# the chunk driver: N = 7000, H = 226 per trajectory -- no plan of the whole batch; the forward kernel takes 512 rows a
# launch (512 + 45), k1_solve_adj 256 (256 + 256 + 45): a ragged last launch in both directions
CHUNKED = (7000, 226, 557)
CHUNKS = {ODEINT: (512, dict(kernel=1, HT=8, HC=2, NW=4, TPW=4, NB=2, G=110, TG=2, ntg=16, nblk=219)),
          ADJOINT: (256, dict(kernel=1, HT=8, HC=2, NW=4, TPW=2, NB=2, G=110, TG=2, ntg=8, nblk=219))}


def control_of(name):
    from phoenix_amd import _lib
    return _lib.CTRL_SHARED if name == "shared" else _lib.CTRL_PER_TRAJECTORY


def plan(op, kernel, N, H, B, control, method="rk4", cus=256):
    """phx_debug_plan as a dict of every field (None: the kernel does not plan the batch); cus = 256 needs no device"""
    from phoenix_amd import _lib
    out = (C.c_longlong * len(pt.FIELDS))()
    if not _lib.load().phx_debug_plan(op, kernel, cus, N, H, B, T, control_of(control), _lib.METHODS[method], 1, out):
        return None
    return dict(zip(pt.FIELDS, (int(v) for v in out)))


def dispatch(op, N, H, B, control, method="rk4", cus=256):
    """(kernel, plan) of the first kernel of the direction that plans the batch in one launch -- forward: k1_solve_fwd;
    backward: k1_solve_adj2, then k1_solve_adj -- or (0, None): the VALU pair"""
    for k in ((1,) if op == ODEINT else (2, 1)):
        d = plan(op, k, N, H, B, control, method, cus)
        if d is not None:
            return k, d
    return 0, None


def check_row(name, cus=256):
    """the plans of GEOMETRY[name] on `cus` compute units, asserted to be the table's; the caller has set the row's env"""
    (N, H, B, control, env), fwd, bwd = GEOMETRY[name]
    got = []
    for op, want in ((ODEINT, fwd), (ADJOINT, bwd)):
        k, d = dispatch(op, N, H, B, control, cus=cus)
        print("%s %s N=%d H=%d B=%d %s %s: kernel %d %s" % (name, "fwd" if op == ODEINT else "bwd", N, H, B, control, env, k,
                                                        d and {f: d[f] for f in WANT + ("lds",)}))
        assert (want is None) == (d is None), (name, op, k, d)
        if want is not None:
            assert dict({f: d[f] for f in WANT}, kernel=k) == want, (name, op, k, d)
            # what test_plans_cpu holds every plan of its sweep to: every workgroup resident, LDS within the budget
            assert d["TG"] * d["G"] <= 256 and d["lds"] <= LDS_BUDGET and d["Bt"] == 16 * d["ntg"], (name, d)
            if control == "shared":
                assert d["TG"] == 1, (name, d)      # one batch group
        got.append((k, d))
    return got


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_geometry_table_on_256_cus(name, monkeypatch):
    for k in pt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in GEOMETRY[name][0][4].items():
        monkeypatch.setenv(k, v)
    check_row(name)
    (N, H, B, control, env), fwd, bwd = GEOMETRY[name]
    for op in (ODEINT, ADJOINT):      # the plan does not depend on which fixed-grid method steps
        assert dispatch(op, N, H, B, control, "euler") == dispatch(op, N, H, B, control, "midpoint") == dispatch(op, N, H, B, control)


def reached(op, **want):
    return [n for n, row in GEOMETRY.items() if row[1 if op == ODEINT else 2] is not None and
            all(row[1 if op == ODEINT else 2][k] == v for k, v in want.items())]


def test_table_reaches_every_instantiation_and_planner_axis():
    """every kernel form and planner axis value the table is there for, by at least one row"""
    f, b = ODEINT, ADJOINT
    # k1_solve_fwd
    assert reached(f, HT=3, NW=4, ntg=1) and reached(f, HT=3, NW=4, ntg=4, TG=1) and reached(f, HT=3, NW=4, TG=2)
    assert [n for n in reached(f, HT=3, NW=4) if GEOMETRY[n][1]["G"] > 32]
    assert reached(f, HT=3, NW=8, TPW=1, TG=1) and reached(f, HT=3, NW=8, TPW=2) and reached(f, HT=3, NW=8, TPW=4)
    assert [n for n in reached(f, HT=3, NW=8) if GEOMETRY[n][1]["TG"] > 1]
    assert reached(f, HT=3, NW=8, NB=2) and reached(f, HT=3, NW=8, NB=3) and reached(f, HT=3, NW=4, NB=3)
    assert reached(f, HT=8, HC=1, TPW=1) and reached(f, HT=8, HC=1, TPW=2, NB=1) and reached(f, HT=8, HC=1, TPW=4)
    assert reached(f, HT=8, HC=1, NB=2, TG=3) and reached(f, HT=8, HC=1, NB=3) and reached(f, HT=8, HC=1, NB=2, TPW=2)
    assert reached(f, HT=7, HC=2, TPW=1) and reached(f, HT=7, HC=2, TPW=4) and reached(f, HT=7, HC=2, TG=2) and reached(f, HT=7, HC=2, NB=2)
    assert reached(f, HT=8, HC=2, TPW=1) and reached(f, HT=8, HC=2, TPW=4) and reached(f, HT=8, HC=2, NB=2)
    assert {48, 49, 128, 129, 224, 226, 256} <= {row[0][1] for row in GEOMETRY.values() if row[0][0] == 45}
    # k1_solve_adj2: the 8-wave form (HT = 3) and the 4-wave form (HT = 8)
    assert reached(b, kernel=2, HT=3, NW=8, ntg=1) and reached(b, kernel=2, HT=3, NW=8, TPW=2) and reached(b, kernel=2, HT=3, NW=8, TPW=4)
    assert reached(b, kernel=2, HT=3, TG=2) and reached(b, kernel=2, HT=3, NB=2, TG=24) and reached(b, kernel=2, HT=3, NB=3)
    assert reached(b, kernel=2, HT=8, NW=4, ntg=1) and reached(b, kernel=2, HT=8, NW=4, ntg=2, TG=1)
    assert reached(b, kernel=2, HT=8, NW=4, TPW=2, ntg=4) and reached(b, kernel=2, HT=8, NW=4, TPW=2, ntg=3)
    assert reached(b, kernel=2, HT=8, NW=4, TPW=4, NB=1) and reached(b, kernel=2, HT=8, TG=2, ntg=2)
    assert reached(b, kernel=2, HT=8, NB=3, TG=5) and reached(b, kernel=2, HT=8, NB=2, TPW=2)
    assert reached(b, kernel=2, HT=3, NW=4) and reached(b, kernel=2, HT=8, NW=8)      # the non-default pairings
    # k1_solve_adj
    assert [n for n in reached(b, kernel=1, HT=3, NW=4, TPW=1) if GEOMETRY[n][2]["G"] > 32]
    assert reached(b, kernel=1, HT=3, TPW=2) and reached(b, kernel=1, HT=3, TPW=4) and reached(b, kernel=1, HT=3, NB=2)
    assert reached(b, kernel=1, HT=3, NW=1, TG=4) and reached(b, kernel=1, HT=3, NW=2, TG=5)
    assert reached(b, kernel=1, HT=8, HC=1, TPW=4) and [n for n in reached(b, kernel=1, HT=8, HC=1) if GEOMETRY[n][0][4]]
    for ht in (7, 8):
        assert reached(b, kernel=1, HT=ht, HC=2, ntg=1, NW=4) and reached(b, kernel=1, HT=ht, HC=2, TPW=1, ntg=4)
        assert reached(b, kernel=1, HT=ht, HC=2, TPW=2) and reached(b, kernel=1, HT=ht, HC=2, TPW=4) and reached(b, kernel=1, HT=ht, HC=2, NB=2)
    assert reached(b, kernel=1, HT=7, HC=2, NW=1) and reached(b, kernel=1, HT=7, HC=2, NW=2)
    # the VALU pair, and the shape rule: at least every second batch is no multiple of 16
    assert [n for n, row in GEOMETRY.items() if row[2] is None and row[1] is not None]      # k1_solve_fwd, then k_solve_adj
    assert [n for n, row in GEOMETRY.items() if row[2] is None and row[1] is None]          # k_solve_fwd and k_solve_adj
    ragged = [row[0][2] % 16 != 0 for row in GEOMETRY.values()]
    assert 2 * sum(ragged) >= len(ragged)
    for n, row in GEOMETRY.items():      # a batch that is a multiple of 16 has a neighbour 3 rows short
        N, H, B, control, env = row[0]
        if B % 16 == 0:
            assert any(r[0][:2] == (N, H) and r[0][2] == B - 3 for r in GEOMETRY.values()), n


def test_no_mfma_kernel_plans_19_shared_tiles_backward(monkeypatch):
    """N = 45, H = 7, B = 300 under shared control: 19 tiles are more than one batch group of either backward kernel
    holds (16: four tiles a wave), so the call falls through to the VALU kernel k_solve_adj -- in silence; this test knows
    that it happens (and the GPU file holds that call to the truth).  256 rows still have a plan, 257 have none."""
    for k in pt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert dispatch(ADJOINT, 45, 7, 300, "shared") == (0, None)
    assert dispatch(ADJOINT, 45, 7, 256, "shared")[0] == 2 and dispatch(ADJOINT, 45, 7, 257, "shared") == (0, None)
    assert plan(ADJOINT, 1, 45, 7, 256, "shared")["TPW"] == 4 and plan(ADJOINT, 1, 45, 7, 257, "shared") is None
    assert dispatch(ODEINT, 45, 7, 300, "shared")[0] == 1
    assert dispatch(ADJOINT, 45, 7, 300, "per_trajectory")[0] == 2      # what a step size runs


def test_chunked_batch_plans(monkeypatch):
    for k in pt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    N, H, B = CHUNKED
    for op, (rows, want) in CHUNKS.items():
        assert dispatch(op, N, H, B, "per_trajectory") == (0, None) and dispatch(op, N, H, 2 * rows, "per_trajectory") == (0, None)
        k, d = dispatch(op, N, H, rows, "per_trajectory")
        assert dict({f: d[f] for f in WANT}, kernel=k) == want, (op, d)
        assert B % rows == 45 and dispatch(op, N, H, B % rows, "per_trajectory")[0] == 1


# ---------------------------------------------------------------------------------------- the condition on the inputs
SEEDS = {name: 2600 + i for i, name in enumerate(sorted(GEOMETRY))}
SMALL = ("h7_b1", "h7_b61", "h7_b100_p", "h49_b37_p", "h129_b61_p", "h226_b61_s", "n1100_b61_p")      # all three methods
PER_SAMPLE = ("ps_h7", "ps_h49", "ps_n1100", "ps_h129")
# one small per_trajectory row per backward kernel form: k1_solve_adj2 with 8 and with 4 waves, k1_solve_adj<3>, <7, CH>
EDGE_ROWS = ("h7_b100_p", "h49_b37_p", "n1100_b61_p", "h129_b61_p")
T5 = np.array(g26.T5, np.float32)


def per_sample_grid(B, seed):
    """t [B, 5]: T5 stretched by another factor in every row, every fourth row decreasing"""
    r = np.random.RandomState(seed)
    t = (r.uniform(0.4, 1.0, (B, 1)) * T5[None] + r.uniform(0.0, 0.3, (B, 1))).astype(np.float32)
    t[::4] = t[::4, ::-1]
    return t


# the time-axis edges: name -> (grid, step_size, adjoint step_size); every one runs rk4 on the rows of EDGE_ROWS
EDGES = {
    # decreasing time turns the decay term -g y into growth: T5 reversed breaks the condition at N = 1100 (e32 6.9e-6 in
    # the Wp gradient's blocks); 0.6 x T5 = (2.7, 2.1, 0.9, 0.6, 0) keeps it
    "dec": ((0.6 * T5[::-1]).astype(np.float32), None, None),
    "dec_h": ((0.6 * T5[::-1]).astype(np.float32), g26.STEP, None),
    "adjstep": (T5, g26.STEP, 0.3),                                                 # the backward solve's own step
    "on_grid": (np.array([0.0, 0.75, 1.5, 3.5, 4.5], np.float32), 0.75, None),      # outputs 1, 2 and 4 ARE grid points
    "h_exceeds_all": (T5, 2.5, None),                                               # one (short) step per interval
    "f64": (np.array(g26.T5, np.float64) * 0.9 + 0.013, None, None),                # no value is a float32
    "f64_h": (np.array(g26.T5, np.float64) * 0.9 + 0.013, 0.3, None),
}


def runs_of(name):
    """(method, step_size) of the runs of a row in the GPU file: rk4, on the small classes euler and midpoint too; a step
    size where the row is planned per trajectory"""
    control = GEOMETRY[name][0][3]
    hs = (None, g26.STEP) if control == "per_trajectory" else (None,)
    return [(m, h) for m in (("euler", "midpoint", "rk4") if name in SMALL else ("rk4",)) for h in hs]


def references(name, method, h, t=None, ah=None, dev="cpu", orc=None, seed=0):
    """inputs, the float64 truth and the float32 references' figures against it (e32) of one run of a row"""
    N, H, B = GEOMETRY[name][0][:3] if name in GEOMETRY else CHUNKED
    t = T5 if t is None else t
    p, y0, G = g26.inputs(N, H, B, SEEDS.get(name, 2599) + 100 * seed, T=t.shape[-1])
    truth = g26.arbiter(p, torch.float64, y0, t, G, method, h, ah, dev)
    ref32 = g26.arbiter(p, torch.float32, y0, t, G, method, h, ah, dev)
    o32 = g26.oracle_ref(orc, p, y0, t, G, method) if orc is not None and g26.oracle_applies(N, H, B, h, ah) else None
    return (p, y0, t, G), truth, g26.e32_of(truth, ref32, o32)


@pytest.mark.parametrize("name, method, h", [(n, m, h) for n in sorted(GEOMETRY) if np.prod(GEOMETRY[n][0][:3]) <= CPU_MAX and
                                             n not in PER_SAMPLE for m, h in runs_of(n)])
def test_inputs_are_well_conditioned(name, method, h, oracle):
    """every figure of both float32 references within TOL_FIXED / 2 of the truth, for every run of the row"""
    _, _, e32 = references(name, method, h, orc=oracle)
    g26.conditioned("%s/%s/h=%s" % (name, method, h), e32)


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edge_inputs_are_well_conditioned(edge, oracle):
    t, h, ah = EDGES[edge]
    assert (t.dtype == np.float64) == edge.startswith("f64")
    if t.dtype == np.float64:
        assert not np.any(t.astype(np.float32).astype(np.float64) == t)
    for name in EDGE_ROWS:
        assert GEOMETRY[name][0][3] == "per_trajectory"      # what a step size plans
        _, _, e32 = references(name, "rk4", h, t=t, ah=ah, orc=oracle, seed=1)
        g26.conditioned("%s/%s" % (name, edge), e32)


@pytest.mark.parametrize("h", [None, 0.3])
@pytest.mark.parametrize("name", PER_SAMPLE)
def test_per_sample_inputs_are_well_conditioned(name, h, oracle):
    B = GEOMETRY[name][0][2]
    t = per_sample_grid(B, SEEDS[name])
    assert B <= 20 and len({float(x) for x in t[:, 1] - t[:, 0]}) == B and (t[::4, 0] > t[::4, 1]).all()
    _, _, e32 = references(name, "rk4", h, t=t, orc=oracle, seed=2)
    g26.conditioned("%s/per-sample/h=%s" % (name, h), e32)


# ---------------------------------------------------------------------------------------- the arbiter against G26
@pytest.fixture(scope="module")
def gold():
    from conftest import load_golden
    return load_golden("g26_fixed_truth")


def test_g26_covers_what_it_is_there_for():
    cases = g26.GOLDEN_CASES
    assert {c[1] for c in cases} == {"euler", "midpoint", "rk4"} and {c[2] for c in cases} == {"inc", "dec"}
    assert {c[3] for c in cases} == {None, 0.75, 0.3} and {c[0][1] for c in cases} == {7, 49}
    assert max(c[0][0] for c in cases) == 97 and max(c[0][2] for c in cases) <= 5
    assert any(c[4] is not None and c[4] != c[3] for c in cases)


@pytest.mark.parametrize("case", g26.GOLDEN_CASES, ids=g26.golden_name)
def test_float64_arbiter_reproduces_g26(gold, case):
    """the truth of the GPU file is the reference's: bar g26.GOLDEN_BAR = 1e-12, the stored dtype being float64 and the
    arithmetic the same in another order (measured: DESIGN.md)"""
    from conftest import relerr, sub
    (N, H, B), method, tname, h, ah = case
    p, y0, t, G = g26.golden_inputs(case)
    c = sub(gold, g26.golden_name(case) + "/")
    assert np.array_equal(c["checksums"], g26.checksums(p))
    assert c["sol"].dtype == np.float64 and t.dtype == np.float64
    got = g26.arbiter(p, torch.float64, y0, t, G, method, h, ah)
    worst = max(relerr(got[k].reshape(c[k].shape), c[k]) for k in g26.QUANT)
    print("%s arbiter vs G26: %.2e" % (g26.golden_name(case), worst))
    assert worst < g26.GOLDEN_BAR
