#!/usr/bin/env python3
"""Diagnostic: the launch plans of the persistent solve kernels over a grid of shapes.
Two builds plan alike when their tables are equal; a planner change shows as the rows it moves.

Without --cus (GPU box: the queries plan for the device's CU count): one line per (environment, N, H, B, control,
method) -- the kernel generation of both directions, their launch counts, the profile region of both directions,
phx_workspace_bytes of both solve ops and phx_odeint_calls_workspace_bytes.

With --cus N (no GPU needed): the plans themselves through phx_debug_plan, for a device of N compute units -- one line
per (environment, kernel, N, H, B, control, method, calls) with every field of the launch geometry, the workspace
layout and the LDS bytes, `-` where the kernel does not plan the shape.  The kernel is the first one of the direction
that plans the batch in one launch; --kernels: every solve kernel of both directions and k1_solve_bp instead, and for
the forward kernels also the several-calls forms.  --golden: the short shape list of tests/golden/solve_plans.txt
instead of the grid.
usage: python tools/plan_table.py [out_file] [--cus N [--kernels] [--golden]]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phoenix_amd import _lib  # noqa: E402

NS = (350, 690, 2000, 3551, 6000, 11165, 14691, 70000)
HS = (8, 40, 48, 64, 100, 120, 128, 130, 200, 256)
BS = (1, 2, 4, 17, 64, 128, 256, 673, 680, 686, 1024, 2048, 4097)
T = 2
ENVS = ((), (("PHX_ADJ", "v1"),), (("PHX_ADJ", "v2"),), (("PHX_ADJ", "v3"),), (("PHX_FWD", "v1"),), (("PHX_V3C", "0"),),
        (("PHX_ENGINE", "v0"),))
# ... and with --cus the switches inside the searches
PLAN_ENVS = ENVS + ((("PHX_V3C_HB", "0"),), (("PHX_V3C_NTG", "4"),), (("PHX_V3C_SPLIT", "0"),), (("PHX_V1_MAXNW", "2"),),
                    (("PHX_ADJ2_NP", "2"),), (("PHX_V3_NB", "2"),))
SWITCHES = sorted({k for env in PLAN_ENVS for k, _ in env})
ODEINT, ADJOINT = 2, 3
KERNELS = ((ODEINT, 3), (ODEINT, 4), (ODEINT, 1), (ADJOINT, 3), (ADJOINT, 4), (ADJOINT, 2), (ADJOINT, 1), (ADJOINT, 5))
CALLS = (2, 7, 300)
# phx_debug_plan's out[] (include/phoenix_hip.h)
FIELDS = ("N", "H", "B", "T", "HT", "NB", "NW", "TPW", "G", "TG", "nblk", "ntg", "Bt", "nvec", "BN", "HC", "Hc", "Bcall", "cntN",
          "res", "hb", "split", "total", "cnt", "part", "zbuf", "part1", "zbuf1", "scratch", "dtheta", "prof", "wimg", "hq",
          "xbytes", "pp", "nparts", "lds")
# --golden: bench.py's four workloads, then the hidden widths, gene counts and batches at which the planners change path
GOLDEN_SHAPES = ((11165, 40, 256), (350, 40, 1024), (2000, 120, 23), (14691, 200, 256)) + \
    tuple((2000, H, 64) for H in (48, 49, 128, 129, 256)) + tuple((N, 40, 64) for N in (32, 33, 70000)) + \
    tuple((350, 40, B) for B in (1, 16, 17, 673, 686, 4097)) + \
    tuple((6000, 200, B) for B in (1, 16, 17, 673, 686, 4097))


def set_env(env, keys=SWITCHES):
    """the planners read the switches from the live environment"""
    for k in keys:
        os.environ.pop(k, None)
    for k, v in env:
        os.environ[k] = v
    return ",".join("%s=%s" % kv for kv in env) or "-"


def plan(lib, op, kernel, cus, N, H, B, ctl, m, calls=1):
    """phx_debug_plan's values as a tuple in the order of FIELDS, None where the kernel does not plan the shape"""
    out = (C.c_longlong * len(FIELDS))()
    return tuple(out) if lib.phx_debug_plan(op, kernel, cus, N, H, B, T, ctl, m, calls, out) else None


def plans(lib, cus, shapes, envs, kernels, methods=range(4)):
    """(tag, op, kernel, N, H, B, control, method, calls, plan()) over the sweep.  kernels: every kernel, and the forward
    ones also with several calls of B rows each; else the first kernel of a direction that plans the batch"""
    for env in envs:
        tag = set_env(env)
        for N, H, B in shapes:
            for ctl in (0, 1):
                for m in methods:
                    served = set()
                    for op, k in KERNELS:
                        if (k == 5 and (m == 3 or ctl == 0 or not kernels)) or (not kernels and op in served):
                            continue   # (k1_solve_bp: a fixed grid has no controller)
                        for calls in ((1,) + CALLS if kernels and op == ODEINT else (1,)):
                            v = plan(lib, op, k, cus, N, H, B * calls, ctl, m, calls)
                            if v is not None:
                                served.add(op)
                            if kernels or v is not None:
                                yield tag, op, k, N, H, B * calls, ctl, m, calls, v
    set_env(())


def plan_lines(*args):
    """the lines of the --cus table"""
    for row in plans(*args):
        yield "%s op=%d k=%d N=%d H=%d B=%d ctl=%d m=%d calls=%d " % row[:9] + (" ".join(map(str, row[9])) if row[9] else "-") + "\n"


def golden_lines(lib, cus=256):
    """tests/golden/solve_plans.txt: every kernel under dopri5 (k1_solve_bp: rk4) and both controls, no switches set; the
    several-calls forms only where a kernel plans them"""
    yield "# cus %d: %s\n" % (cus, " ".join(FIELDS))
    for line in plan_lines(lib, cus, GOLDEN_SHAPES, ((),), True, (2, 3)):
        f = line.split()
        if (f[7] == "m=2") == (f[2] == "k=5") and (f[8] == "calls=1" or f[9] != "-"):
            yield line


def device_table(lib, out):
    keys = sorted({k for env in ENVS for k, _ in env})   # no other variable of the caller's environment is touched
    lib.phx_debug_profile_region.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    out.write("# cus %d\n" % lib.phx_device_cus())
    for env in ENVS:
        tag = set_env(env, keys)
        for N in NS:
            for H in HS:
                for B in BS:
                    ws = (lib.phx_workspace_bytes(ODEINT, N, H, B, T), lib.phx_workspace_bytes(ADJOINT, N, H, B, T))
                    calls = tuple(lib.phx_odeint_calls_workspace_bytes(N, H, B, T, c) for c in (2, B))
                    for ctl in (0, 1):
                        regions = []
                        for op in (ODEINT, ADJOINT):
                            off, nwg, plan6 = C.c_size_t(0), C.c_int(0), (C.c_int * 6)()
                            rc = lib.phx_debug_profile_region(op, N, H, B, T, ctl, C.byref(off), C.byref(nwg), plan6)
                            regions.append("%d:%d:%d:%s" % (rc, off.value if rc == 0 else 0, nwg.value if rc == 0 else 0,
                                                            ".".join(str(x) for x in plan6) if rc == 0 else "-"))
                        for m in range(4):
                            out.write("%s N=%d H=%d B=%d ctl=%d m=%d kern=%d/%d launches=%d/%d region=%s/%s ws=%d/%d calls_ws=%d/%d\n" % (
                                tag, N, H, B, ctl, m, lib.phx_debug_forward_kernel_m(N, H, B, T, ctl, m),
                                lib.phx_debug_adjoint_kernel_m(N, H, B, T, ctl, m),
                                lib.phx_debug_solve_launches(ODEINT, N, H, B, T, ctl, m),
                                lib.phx_debug_solve_launches(ADJOINT, N, H, B, T, ctl, m), regions[0], regions[1],
                                ws[0], ws[1], calls[0], calls[1]))
    set_env((), keys)


def main():
    args = sys.argv[1:]
    cus = int(args.pop(args.index("--cus") + 1)) if "--cus" in args else 0
    flags = {a for a in args if a.startswith("--")}
    files = [a for a in args if not a.startswith("--")]
    lib = _lib.load()
    out = open(files[0], "w") if files else sys.stdout
    if cus <= 0:
        device_table(lib, out)
    elif "--golden" in flags:
        out.writelines(golden_lines(lib, cus))
    else:
        out.write("# cus %d: %s\n" % (cus, " ".join(FIELDS)))
        out.writelines(plan_lines(lib, cus, [(N, H, B) for N in NS for H in HS for B in BS], PLAN_ENVS, "--kernels" in flags))
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
