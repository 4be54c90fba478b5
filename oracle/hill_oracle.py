"""TEST INFRASTRUCTURE ONLY (see oracle/phx_oracle.h): reference semantics of the Hill-kinetics rate expressions.

The expressions in `ode_system_functions_*.csv` are R source text emitted by GraphGRN_core.R:425-486; their only
function is `fAct` (GraphGRN_core.R:431-436) and their arithmetic is also valid Python, so the reference value of a
rate is Python's own evaluation of the shipped string in fp64.  Trajectories: scipy's LSODA at tight tolerances
(the reference integrates with deSolve::ode, which is lsoda).  Pinned only against the shipped expression files --
the R run itself (RNG draws, lsoda step sequence) cannot be reproduced in this image."""
import numpy as np


def fAct(TF, EC50=0.5, n=1.39):
    B = (EC50 ** n - 1) / (2 * EC50 ** n - 1)
    K_n = B - 1
    return B * TF ** n / (K_n + TF ** n)


def fAct0(TF, EC50=0.5, n=1.39):
    """`fAct` continued to TF <= 0 by TF^n := 0, which is what the device interpreter (csrc/phx_hill.inc) and
    `interpret_programs` below define there; R and `fAct` give NaN for a negative TF and a fractional n.  For TF > 0
    the operations, and so the bits, are those of `fAct`.  TF: an array or a Python float."""
    B = (EC50 ** n - 1) / (2 * EC50 ** n - 1)
    K_n = B - 1
    if isinstance(TF, float):
        tn = TF ** n if TF > 0 else 0.0
    else:
        TF = np.asarray(TF, np.float64)
        tn = np.where(TF > 0, np.abs(TF) ** n, 0.0)
    return B * tn / (K_n + tn)


def compile_rhs(names, expressions, fact=fAct):
    """`rhs` with the expression strings compiled once: returns f(x, rowwise=False) -> rates, for callers that evaluate
    many states of one network (an RK4 restatement); `fact` is the function the strings' `fAct` is bound to.
    rowwise=True evaluates the strings once per row of x on Python floats instead of once on numpy columns: the same float64
    arithmetic, several times faster for a handful of rows (`fact` must take a float then)."""
    codes = [None if e.strip() == "input gene" else compile(e, "<eqn %s>" % names[g], "eval")
             for g, e in enumerate(expressions)]
    live = [(g, c) for g, c in enumerate(codes) if c is not None]

    def f(x, rowwise=False):
        x = np.asarray(x, np.float64)
        out = np.zeros_like(x)
        if rowwise:
            xr, outr = x.reshape(-1, x.shape[-1]), out.reshape(-1, x.shape[-1])
            for b in range(xr.shape[0]):
                env = dict(zip(names, xr[b].tolist()))
                env["fAct"] = fact
                outr[b, [g for g, _ in live]] = [eval(c, {"__builtins__": {}}, env) for _, c in live]
            return out
        env = {n: x[..., i] for i, n in enumerate(names)}
        env["fAct"] = fact
        for g, c in live:
            out[..., g] = eval(c, {"__builtins__": {}}, env)
        return out

    return f


def rhs(names, expressions, x, fact=fAct):
    """rates of every gene at the states x [..., N] ('input gene' rows: 0)."""
    return compile_rhs(names, expressions, fact)(x)


def simulate(names, expressions, x0, times, rtol=1e-10, atol=1e-12):
    from scipy.integrate import solve_ivp
    codes = [None if e.strip() == "input gene" else compile(e, "<eqn>", "eval") for e in expressions]

    def f(_t, y):
        env = dict(zip(names, y))
        env["fAct"] = fAct
        return [0.0 if c is None else eval(c, {"__builtins__": {}}, env) for c in codes]

    sol = solve_ivp(f, (times[0], times[-1]), np.asarray(x0, np.float64), t_eval=times, method="LSODA", rtol=rtol, atol=atol)
    return sol.y.T


def interpret_programs(code, consts, off, length, x, dtype=np.float64):
    """fp64 interpreter of the postfix programs phoenix_amd.simulator compiles (same opcodes as csrc/phx_hill.inc):
    checks the COMPILER against `rhs` above without a GPU.  dtype=np.float32 runs every operation in fp32 (states and
    constants rounded first, as the device holds them): the rounding error a correct fp32 interpreter may show."""
    x = np.asarray(x, dtype)
    consts = np.asarray(consts, dtype)
    out = np.zeros_like(x)
    for g in range(len(off)):
        st = []
        for op, arg in code[off[g]: off[g] + length[g]]:
            if op == 0:
                st.append(np.full(x.shape[:-1], consts[arg]))
            elif op == 1:
                st.append(x[..., arg])
            elif op == 6:
                st[-1] = -st[-1]
            elif op == 7:
                b, k, n = consts[arg: arg + 3]
                tn = np.where(st[-1] > 0, np.abs(st[-1]) ** n, dtype(0))
                st[-1] = b * tn / (k + tn)
            else:
                r = st.pop()
                st[-1] = st[-1] + r if op == 2 else st[-1] - r if op == 3 else st[-1] * r if op == 4 else st[-1] / r
        if st:
            out[..., g] = st[0]
    return out
