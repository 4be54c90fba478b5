"""The float64 truth of the fixed-grid solves (`odeint_adjoint(method="euler" | "midpoint" | "rk4")`, with and without
options["step_size"]) and what tests/test_fixed_grid_cpu.py, tests/test_fixed_grid_truth_gpu.py and the generator of
golden G26 (tests/golden/make_golden_fixed_truth.py) share: the seeded inputs, the arbiter, the error figures and the bar.

The arbiter is the continuous adjoint in plain torch: TorchNet (tests/test_backprop_gpu.py, ODENet.forward restated in the
dtype of its tensors) solved by phoenix_amd.generic.odeint_adjoint -- the forward fixed grid, then the augmented system of
adjoint.py stepped by the same method one interval at a time.  A fixed grid has no step controller, so the same steps in
float64 are the same discrete operation: whatever a kernel differs from them by above float32 rounding is its error.
Golden G26 pins the float64 arbiter to the reference's own odeint_adjoint (test_fixed_grid_cpu.py).

Figures, per case and quantity (figures()):
  <k>        global relerr, max |a - b| / max |b|, of sol, grad_y0 and the six parameter gradients
  row:<k>    worst trajectory row of sol and grad_y0, the row's error normalised by the row's OWN largest truth entry
  blk:<k>    worst block of 32 genes -- columns of the Ws and Wp gradients, rows of Wa's, entries of g's -- normalised by
             the block's own largest truth entry; blocks are the kernels' nblk = ceil(N / 32), the ragged last one included
Bar of every figure (hold()): err < max(TOL_FIXED, 2 e32), e32 = the same figure of the float32 references against the
truth, the larger of the torch arbiter's and the C oracle's; margin and TOL_FIXED are test_backprop_geometry_gpu.hold's.
Nothing in it comes from the code under test.  Condition on the inputs (conditioned()): every e32 <= TOL_FIXED / 2, so
that the bar IS TOL_FIXED and no ill-conditioned problem widens it.

Inputs (inputs()): drawn as test_backprop_geometry_gpu.inputs draws them -- weights N(0, STD), start states beta(2, 2)
plus a gene offset, clipped to [0, 1] -- with cotangents of size 1 / (B N) at every output time (the scale of a mean
loss), on the time grid T5 = SCALE x (0, 2, 3, 7, 9).  STD = 0.05 is that of the k1_solve_bp tests, lowered for large
networks (std_for()); at SCALE = 1 (their grid) the rk4 interval of length 4 breaks the condition in float32 (e32 up to
2.3e-5 at N = 1100, H = 7, B = 64), at SCALE = 0.5 it holds in every case of the table (DESIGN.md has the measured e32).
The small gene count of the table is 45, not 33: a ragged last block of ONE gene has no "own largest entry" to speak of
(dL/dg of a single gene is a sum over rows and times that can cancel to nothing, e32 1.7e-4 at N = 33, H = 226, B = 64);
13 genes do, and 45 plans exactly as 33 does.

The C oracle (oracle.odeint_per_sample / adjoint_backward_per_sample) takes one step per interval and has no step size:
it is the second float32 reference of the cases without one and is left out of the stepped cases.  It is plain scalar
C, so it is also left out above ORACLE_MAX = N x H x B where it would take longer than the rest of a test."""
import numpy as np
import torch

KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")
QUANT = ("sol", "grad_y0") + tuple("grad_" + k for k in KEYS)
TOL_FIXED = 1e-5      # the project's fixed-grid bar (tests/test_backprop_gpu.py)
MARGIN = 2.0          # test_backprop_geometry_gpu.hold
STD = 0.05
SCALE = 0.5
T5 = tuple(SCALE * x for x in (0.0, 2.0, 3.0, 7.0, 9.0))
STEP = 0.75          # on T5 = (0, 1, 1.5, 3.5, 4.5): divides no interval (a short last sub-step) and exceeds the second
ORACLE_MAX = 33 * 256 * 300


def params(N, H, seed, std=STD, neg=0.1):
    """tests/test_backprop_gpu.py rand_params"""
    r = np.random.RandomState(seed)
    g = r.rand(N).astype(np.float32)
    g[r.rand(N) < neg] *= -1
    return {"Ws": (r.randn(H, N) * std).astype(np.float32), "bs": r.uniform(-.2, .2, H).astype(np.float32),
            "Wp": (r.randn(H, N) * std).astype(np.float32), "bp": r.uniform(-.2, .2, H).astype(np.float32),
            "Wa": (r.randn(N, 2 * H) * std).astype(np.float32), "g": g}


def std_for(N, H):
    """STD, lowered where the network is large: the Jacobian of the right-hand side is about Wa diag Ws, of spectral
    radius about sqrt(N H) std^2, and the 4.5 time units of T5 amplify a rounding error by exp(4.5 x radius); the radius
    is kept to 0.25 (a factor 3), which binds from N H = 10 000 on"""
    return min(STD, (0.25 / (N * H) ** 0.5) ** 0.5)


def inputs(N, H, B, seed, T=len(T5)):
    """parameters, start states [B, N] and cotangents [T, B, N] of size 1 / (B N)"""
    p = params(N, H, seed, std=std_for(N, H))
    r = np.random.RandomState(seed + 1)
    y0 = np.clip(r.beta(2, 2, size=(B, N)) + r.uniform(-0.25, 0.25, size=(1, N)), 0, 1).astype(np.float32)
    G = (r.randn(T, B, N) / (B * N)).astype(np.float32)
    return p, y0, G


def _solve(net, dev, dtype, y0, t, G, method, h, ah):
    from phoenix_amd import generic
    for q in net.parameters():
        q.grad = None
    y0r = torch.from_numpy(y0).to(dev, dtype).requires_grad_(True)
    sol = generic.odeint_adjoint(net, y0r, torch.from_numpy(t).to(dev), 1e-7, 1e-9, method, {"step_size": h} if h else {},
                                 1e-7, 1e-9, method, None, (ah if ah else h) or None)
    (sol * torch.from_numpy(G).to(dev, dtype)).sum().backward()
    out = {"sol": sol.detach().cpu().numpy(), "grad_y0": y0r.grad.cpu().numpy()}
    out.update({"grad_" + k: getattr(net, k).grad.cpu().numpy().copy() for k in KEYS})
    return out


def arbiter(p, dtype, y0, t, G, method, h=None, ah=None, dev="cpu"):
    """sol [T, B, N], grad_y0 [B, N] and the six parameter gradients of sum(G * odeint_adjoint(TorchNet, y0, t)) in
    `dtype`.  t [T] in its own dtype (the step grid of `h` is formed in it, as the engine and the reference form it), or
    [B, T]: one grid per row -- generic takes a 1-D t, so the rows are solved one by one and their parameter gradients
    summed.  h: options["step_size"]; ah: adjoint_options["step_size"] (None: the forward's)."""
    from test_backprop_gpu import TorchNet
    net = TorchNet(p, torch.device(dev), dtype)
    t = np.asarray(t)
    if t.ndim == 1:
        return _solve(net, dev, dtype, y0, t, G, method, h, ah)
    rows = [_solve(net, dev, dtype, y0[b:b + 1], t[b], G[:, b:b + 1], method, h, ah) for b in range(len(t))]
    out = {"sol": np.concatenate([x["sol"] for x in rows], 1), "grad_y0": np.concatenate([x["grad_y0"] for x in rows])}
    out.update({"grad_" + k: sum(x["grad_" + k].astype(np.float64) for x in rows).astype(rows[0]["grad_" + k].dtype)
                for k in KEYS})
    return out


def oracle_applies(N, H, B, h, ah):
    return not h and not ah and N * H * B <= ORACLE_MAX


def oracle_ref(orc, p, y0, t, G, method):
    """the same quantities from the float32 C oracle, one step per interval; t [T] or [B, T]"""
    net = orc.Net(*[p[k] for k in KEYS])
    t = np.asarray(t)
    tb = t if t.ndim == 2 else np.tile(t[None], (len(y0), 1))
    sol = orc.odeint_per_sample(net, y0, tb, method=method)                                   # [B, T, N]
    adj, gr = orc.adjoint_backward_per_sample(net, tb, sol, np.ascontiguousarray(G.transpose(1, 0, 2)), method=method)
    out = {"sol": sol.transpose(1, 0, 2), "grad_y0": adj}
    out.update({"grad_" + k: gr[k] for k in KEYS})
    return out


def _worst(a, b, axes):
    """largest over the slices of max |a - b| / max |b|, both maxima taken over `axes` of a slice"""
    num = np.abs(a - b).max(axis=axes)
    den = np.maximum(np.abs(b).max(axis=axes), 1e-30)
    return float((num / den).max())


def _blocks(x, axis, N):
    """x with its gene axis (length N) first and split into ceil(N / 32) blocks: [nblk, 32, rest], the ragged last block
    padded with zeros (a zero changes neither maximum)"""
    x = np.moveaxis(x, axis, 0).reshape(N, -1)
    nblk = -(-N // 32)
    pad = np.zeros((nblk * 32, x.shape[1]))
    pad[:N] = x
    return pad.reshape(nblk, 32, -1)


def figures(got, truth):
    """every figure of the module docstring: {name: error}"""
    f = {}
    a = {k: np.asarray(got[k], np.float64).reshape(np.shape(truth[k])) for k in QUANT}
    b = {k: np.asarray(truth[k], np.float64) for k in QUANT}
    N = b["grad_y0"].shape[-1]
    for k in QUANT:
        f[k] = _worst(a[k][None], b[k][None], tuple(range(1, b[k].ndim + 1)))
    f["row:sol"] = _worst(a["sol"], b["sol"], (0, 2))
    f["row:grad_y0"] = _worst(a["grad_y0"], b["grad_y0"], (1,))
    for k, axis in (("Ws", 1), ("Wp", 1), ("Wa", 0), ("g", 0)):
        x, y = a["grad_" + k].reshape(b["grad_" + k].shape), b["grad_" + k]
        if k == "g":
            x, y = x.reshape(-1), y.reshape(-1)
        f["blk:" + k] = _worst(_blocks(x, axis, N), _blocks(y, axis, N), (1, 2))
    return f


def e32_of(truth, *refs32):
    """the float32 references' own figures against the truth: per figure the largest over the references"""
    fs = [figures(r, truth) for r in refs32 if r is not None]
    return {k: max(f[k] for f in fs) for k in fs[0]}


def bar(e32, k):
    return max(TOL_FIXED, MARGIN * e32[k])


def conditioned(tag, e32):
    """the condition on the inputs: every figure of the float32 references <= TOL_FIXED / 2"""
    worst = max(e32, key=e32.get)
    print("%s e32 worst %.2e (%s)" % (tag, e32[worst], worst))
    assert e32[worst] <= TOL_FIXED / 2, (tag, worst, e32[worst])


def hold(tag, got, truth, e32):
    """print every figure with its e32, then assert every bar"""
    errs = figures(got, truth)
    for k in errs:
        print("%s %-12s err=%.2e e32=%.2e err/bar=%.3f" % (tag, k, errs[k], e32[k], errs[k] / bar(e32, k)))
    k = max(errs, key=lambda k: errs[k] / bar(e32, k))
    print("%s worst err/bar %.3f (%s)" % (tag, errs[k] / bar(e32, k), k))
    for k in errs:
        assert errs[k] < bar(e32, k), (tag, k, errs[k], e32[k])
    return errs


# ---- golden G26 (tests/golden/make_golden_fixed_truth.py): ((N, H, B), method, grid, step_size, adjoint step_size)
GOLDEN_GRIDS = {"inc": np.array(T5, np.float64), "dec": np.array(T5[::-1], np.float64)}
GOLDEN_CASES = tuple(((33, 7, 3), m, g, h, None) for m in ("euler", "midpoint", "rk4") for g in ("inc", "dec")
                     for h in (None, 0.75, 0.3)) + (
    ((97, 7, 5), "rk4", "dec", 0.3, None), ((97, 7, 5), "euler", "inc", 0.75, 0.3), ((64, 49, 2), "midpoint", "dec", 0.75, None),
    ((97, 49, 5), "rk4", "inc", None, None), ((97, 49, 5), "rk4", "inc", 0.75, 0.3), ((97, 49, 5), "midpoint", "dec", 0.3, None))
# storage is float64 and the arithmetic is the same in another order: sums of O(100) float64 terms, 2^-53 each
GOLDEN_BAR = 1e-12


def golden_name(case):
    (N, H, B), method, tname, h, ah = case
    return "n%d_h%d_b%d/%s/%s/%s/%s" % (N, H, B, method, tname, "none" if h is None else repr(h), "none" if ah is None else repr(ah))


def golden_inputs(case):
    """parameters, y0 [B, N], the float64 grid and cotangents [T, B, N] of a golden case"""
    (N, H, B), method, tname, h, ah = case
    p, y0, G = inputs(N, H, B, 2600 + N + H)
    return p, y0, GOLDEN_GRIDS[tname], G


def checksums(p):
    """[6, 2] float64: sum and sum of squares of every parameter array"""
    return np.array([[np.sum(p[k], dtype=np.float64), np.sum(p[k].astype(np.float64) ** 2)] for k in KEYS])
