#!/usr/bin/env python3
"""Diagnostic (GPU box: planning reads the CU count): the launch plans of the persistent solve kernels over a grid of
shapes, one line per (environment, N, H, B, control, method) -- the kernel generation of both directions, their launch
counts, the profile region of both directions, phx_workspace_bytes of both solve ops and phx_odeint_calls_workspace_bytes.
Two builds plan alike when their tables are equal; a planner change shows as the rows it moves.
usage: python tools/plan_table.py [out_file]"""
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
SWITCHES = ("PHX_ADJ", "PHX_FWD", "PHX_V3C", "PHX_ENGINE")
ODEINT, ADJOINT = 2, 3


def main():
    lib = _lib.load()
    lib.phx_debug_profile_region.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    for k in SWITCHES:
        os.environ.pop(k, None)
    out.write("# cus %d\n" % lib.phx_device_cus())
    for env in ENVS:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in env:
            os.environ[k] = v   # the planners read the switches from the live environment
        tag = ",".join("%s=%s" % kv for kv in env) or "-"
        for N in NS:
            for H in HS:
                for B in BS:
                    ws = (lib.phx_workspace_bytes(ODEINT, N, H, B, T), lib.phx_workspace_bytes(ADJOINT, N, H, B, T))
                    calls = tuple(lib.phx_odeint_calls_workspace_bytes(N, H, B, T, c) for c in (2, B))
                    for ctl in (0, 1):
                        regions = []
                        for op in (ODEINT, ADJOINT):
                            off, nwg, plan = C.c_size_t(0), C.c_int(0), (C.c_int * 6)()
                            rc = lib.phx_debug_profile_region(op, N, H, B, T, ctl, C.byref(off), C.byref(nwg), plan)
                            regions.append("%d:%d:%d:%s" % (rc, off.value if rc == 0 else 0, nwg.value if rc == 0 else 0,
                                                            ".".join(str(x) for x in plan) if rc == 0 else "-"))
                        for m in range(4):
                            out.write("%s N=%d H=%d B=%d ctl=%d m=%d kern=%d/%d launches=%d/%d region=%s/%s ws=%d/%d calls_ws=%d/%d\n" % (
                                tag, N, H, B, ctl, m, lib.phx_debug_forward_kernel_m(N, H, B, T, ctl, m),
                                lib.phx_debug_adjoint_kernel_m(N, H, B, T, ctl, m),
                                lib.phx_debug_solve_launches(ODEINT, N, H, B, T, ctl, m),
                                lib.phx_debug_solve_launches(ADJOINT, N, H, B, T, ctl, m), regions[0], regions[1],
                                ws[0], ws[1], calls[0], calls[1]))
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
