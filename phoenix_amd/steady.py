"""Steady states (attractors) of a PHOENIX ODENet by implicit relaxation.

On the genes that move, f(y) = relu(g) (Wa h(y) - y) with h(y) = [Ws a(y) + bs ; exp(Wp l(y) + bp)]: the Jacobian is a diagonal
plus a product through the 2H-wide hidden vector, so a linearly implicit (Rosenbrock-Euler) step of pseudo-time length tau,
    m = tau g+ / (1 + tau g+),   delta = m (r + Wa x),   (I - S) x = w,   S = C(y) diag(m) Wa,   w = C(y) (m r),   r = Wa h(y) - y
costs one contraction over the genes (phx_reduced_jacobian, the MFMA kernel of phx_steady.hip), two RHS-sized passes and a
2H x 2H dense solve.  With tau small the step follows the ODE and stays in the basin of y0; as tau grows it becomes Newton's.
`steady_states_reference` is the same iteration in numpy, without a GPU.

`steady_states(differentiable=True)` carries a gradient (section 8q): the steady state satisfies P r(y*) = 0, (I - P) y* =
(I - P) y0 with P = diag(1 on the moving genes), so by the implicit function theorem, with gy = dL/dy*,
    b = Wa^T (m gy),   (I - S^T) q = b,   u = gy + C^T q,   lam = m u,   dL/dy0 = (1 - m) u
and the parameter gradients are the outer products of (lam, hid), (q, a) and (q v, l) summed over the rows: one transposed
2H x 2H solve per row and RHS-sized passes, no time integration (phx_steady_adj.hip).  `steady_states_adjoint_reference` is
the same in numpy.

`steady_state_response` is the network of total effects at the fixed points (section 8r): on the moving genes r(y) + u = 0,
so R = dy*/du = M + M Wa Z C M with Z = (I - S)^-1 and M = diag(1 on the moving genes) -- every regulator's answer from one
2H x 2H inverse per state, reduced over the states by a kernel that never forms an N x N temporary (phx_steady_resp.hip).
`steady_state_response_reference` is the same in numpy."""
import collections
import math

import numpy as np
import torch

from . import engine
from .odeint import _clamp_list
from .odenet import params_of

SteadyStates = collections.namedtuple("SteadyStates", ("y", "residual", "iterations", "status", "tau", "reduced"))
KnockoutSteadyStates = collections.namedtuple("KnockoutSteadyStates", ("genes", "base", "knockouts", "shift", "magnitude"))
SteadyAdjoint = collections.namedtuple("SteadyAdjoint", ("y0", "Ws", "bs", "Wp", "bp", "Wa", "g", "lam", "q", "info"))
SteadyResponse = collections.namedtuple("SteadyResponse", ("regulators", "response", "scores", "info"))

CONVERGED, MAX_ITER, SINGULAR = 0, 1, 2      # SteadyStates.status
MAX_ROWS = 32768                             # rows of one pass of the iteration: more are solved in blocks
SOLVE_BYTES = 256 << 20                      # ... and so are rows whose dense systems would take more workspace than this
NOT_CONVERGED = -2                           # last_backward_info(): the row's forward status was not CONVERGED


def _check_control(name, tol, max_iter, tau0):
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol >= 0 or math.isinf(tol):
        raise ValueError("%s: tol must be a finite number >= 0, got %r" % (name, tol))
    if isinstance(max_iter, bool) or not hasattr(max_iter, "__index__") or int(max_iter) < 0:
        raise ValueError("%s: max_iter must be an integer >= 0, got %r" % (name, max_iter))
    if isinstance(tau0, bool) or not isinstance(tau0, (int, float)) or not tau0 > 0:
        raise ValueError("%s: tau0 must be a positive number (inf: plain Newton), got %r" % (name, tau0))


def _rows(name, y, N):
    """y as [B, N] float32 rows (checked on the host)"""
    if not torch.is_tensor(y) or y.dtype != torch.float32 or y.shape[-1] != N or y.dim() not in (2, 3) or \
            (y.dim() == 3 and y.shape[1] != 1) or y.shape[0] < 1:
        raise ValueError("%s: the states must be float32 [B, %d] or [B, 1, %d], got %s" %
                         (name, N, N, (y.dtype, tuple(y.shape)) if torch.is_tensor(y) else type(y).__name__))
    return y.detach().reshape(y.shape[0], N)


def _held_sets(name, clamp, B, N):
    return [()] * B if clamp is None else _clamp_list(clamp, B, N, who=name, unit="row")


def _moving(g, sets, B, device):
    """bool [B, N]: gene n moves in row b -- relu(g) > 0 and n is not in the row's held set"""
    free = (g.detach().reshape(1, -1) > 0).repeat(B, 1)
    rows = [b for b, s in enumerate(sets) for _ in s]
    if rows:
        free[torch.tensor(rows, device=device), torch.tensor([k for s in sets for k in s], device=device)] = False
    return free


def _setup(name, odenet, y, clamp):
    """host checks first, then the GPU requirement -> (Params, y [B, N] contiguous, moving [B, N] bool, relu(g) [N])"""
    tensors = params_of(odenet)
    N = tensors[0].shape[1]
    y2 = _rows(name, y, N)
    sets = _held_sets(name, clamp, y2.shape[0], N)
    engine._require_gpu(tensors[0], "odenet")
    engine._require_gpu(y2, "y")
    p = engine.params_cached(*tensors)
    free = _moving(p.g, sets, y2.shape[0], y2.device)
    return p, y2.contiguous(), free, torch.relu(p.g)


def reduced_jacobian(odenet, y, weight=None, clamp=None):
    """S [B, 2H, 2H] float32 on the device, S_b = C(y_b) diag(m_b) Wa with m = `weight` ([N] or [B, N], default 1) on the genes
    that move in row b (`clamp` as in `steady_states`) and 0 on the others: the 2H x 2H matrix whose spectrum is that of the
    Jacobian's non-diagonal part on the moving genes.  At a steady state with unit weights, an eigenvalue of S near 1 says
    how close the fixed point is to a bifurcation.  One call of phx_reduced_jacobian."""
    with torch.no_grad():
        p, y2, free, _ = _setup("reduced_jacobian", odenet, y, clamp)
        m = free.to(torch.float32)
        if weight is not None:
            if not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.shape not in ((p.N,), tuple(y2.shape)):
                raise ValueError("reduced_jacobian: weight must be float32 [%d] or %s" % (p.N, tuple(y2.shape)))
            m = torch.where(free, weight.to(y2.device).expand_as(m), m.new_zeros(()))
        return engine.reduced_jacobian(p, y2, m.contiguous())[0]


def _iterate(p, y, free, gpos, tol, max_iter, tau0):
    """the iteration on the rows of y; control per row on the device, nothing is read back"""
    B, dev = y.shape[0], y.device
    zero, one = y.new_zeros(()), y.new_ones(())
    gf = torch.where(free, gpos.reshape(1, -1), zero)

    def rho_of(r):
        return torch.where(free, r.abs(), zero).amax(dim=1)       # (amax hands a NaN on)

    r = engine.steady_residual(p, y)[1]
    rho = rho_of(r)
    tau = torch.full((B,), float(tau0), dtype=torch.float32, device=dev)
    status = torch.where(rho <= tol, CONVERGED, MAX_ITER).to(torch.int32)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    for _ in range(int(max_iter)):
        active = status == MAX_ITER
        tg = tau.unsqueeze(1) * gf
        m = torch.where(free & active.unsqueeze(1), torch.where(torch.isinf(tg), one, tg / (1 + tg)), zero)
        S, w, _hid = engine.reduced_jacobian(p, y, m, r)
        x, info = engine.steady_solve(S, w)
        yc = engine.steady_update(p, y, m, r, x)
        rc = engine.steady_residual(p, yc)[1]
        rhoc = rho_of(rc)
        bad = active & (info != 0)
        ok = active & ~bad & torch.isfinite(rhoc) & (rhoc <= 2 * rho)
        rejected = active & ~bad & ~ok
        tau = torch.where(ok, tau * torch.clamp(rho / rhoc, 2.0, 10.0), torch.where(rejected, tau / 4, tau))
        y = torch.where(ok.unsqueeze(1), yc, y)
        r = torch.where(ok.unsqueeze(1), rc, r)
        rho = torch.where(ok, rhoc, rho)
        its = its + active.to(torch.int32)
        status = torch.where(bad, SINGULAR, torch.where(ok & (rhoc <= tol), CONVERGED, status)).to(torch.int32)
    return y, rho, its, status, tau


def _block_rows(p):
    return max(1, min(MAX_ROWS, SOLVE_BYTES // (32 * p.H * p.H)))      # the dense solve holds (2H)^2 doubles per row


def _relax(p, y, free, gpos, tol, max_iter, tau0):
    """`_iterate` on all rows, in blocks of `_block_rows` -> (y, rho, its, status, tau)"""
    step = _block_rows(p)
    parts = [_iterate(p, y[b0:b0 + step], free[b0:b0 + step], gpos, float(tol), max_iter, tau0)
             for b0 in range(0, y.shape[0], step)]
    y, rho, its, status, tau = (torch.cat(c) for c in zip(*parts)) if len(parts) > 1 else parts[0]
    if max_iter == 0:
        y = y.clone()
    return y, rho, its, status, tau


_last_info = None


def last_backward_info():
    """info [B] int32 on the device of the most recent backward pass through `steady_states(differentiable=True)` (None
    before the first): 0 the row's gradient was used, -2 (`NOT_CONVERGED`) its forward status was not CONVERGED, otherwise
    phx_steady_solve's info of the transposed system (k + 1: no pivot in column k, -1: a non-finite solution) -- the row
    sits at a bifurcation.  The backward pass does not synchronise; reading this tensor does."""
    return _last_info


class _SteadyFn(torch.autograd.Function):
    """y* of `steady_states` with the implicit adjoint as its backward (once differentiable)"""

    @staticmethod
    def forward(ctx, y0, ctl, ws, bs, wp, bp, wa, g):
        p, y, free, gpos, tol, max_iter, tau0 = ctl
        out = _relax(p, y, free, gpos, tol, max_iter, tau0)
        ctx.set_materialize_grads(False)
        ctx.phx_params = p
        ctx.phx_versions = tuple(x._version for x in (ws, bs, wp, bp, wa, g))
        ctx.phx_y0_shape = y0.shape
        ctx.save_for_backward(out[0], free, out[3], ws, bs, wp, bp, wa, g)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, *_unused):
        global _last_info
        if gy is None:
            return (None,) * 8
        y, free, status, ws, bs, wp, bp, wa, g = ctx.saved_tensors
        p = ctx.phx_params
        if ctx.phx_versions != tuple(x._version for x in (ws, bs, wp, bp, wa, g)):
            p = engine.params_cached(ws, bs, wp, bp, wa, g)   # parameters were modified in place since forward
        need_p = any(ctx.needs_input_grad[2:8])
        gy = gy.reshape(y.shape).contiguous()
        zero = y.new_zeros(())
        step, grads, gy0s, infos = _block_rows(p), None, [], []
        for b0 in range(0, y.shape[0], step):
            yb, gb, fb = y[b0:b0 + step], gy[b0:b0 + step], free[b0:b0 + step]
            conv = status[b0:b0 + step] == CONVERGED
            S, _w, hid = engine.reduced_jacobian(p, yb, fb.to(torch.float32))
            b = engine.steady_adjoint_project(p, fb.to(torch.float32), gb)
            q, info = engine.steady_solve(S.transpose(1, 2).contiguous(), b)
            # a row that is no fixed point, or whose transposed system is singular, has no gradient: m and q are zeroed
            valid = (conv & (info == 0)).unsqueeze(1)
            m = (fb & valid).to(torch.float32)
            q = torch.where(valid, q, zero)
            lam, gy0 = engine.steady_adjoint_back(p, yb, m, gb, q, hid)
            gy0s.append(torch.where(valid, gy0, zero))
            infos.append(torch.where(conv, info, NOT_CONVERGED).to(torch.int32))
            if need_p:       # (the state and the hidden vector of such a row may be non-finite: 0 x them must stay 0)
                grads = engine.steady_param_grads(p, torch.where(valid, yb, zero), lam, q, torch.where(valid, hid, zero), grads)
        _last_info = torch.cat(infos) if len(infos) > 1 else infos[0]
        gy0 = (torch.cat(gy0s) if len(gy0s) > 1 else gy0s[0]).reshape(ctx.phx_y0_shape) if ctx.needs_input_grad[0] else None
        return (gy0, None) + (tuple(grads.as_reference_layout(g.shape)) if need_p else (None,) * 6)


def steady_states(odenet, y0, clamp=None, tol=1e-5, max_iter=50, tau0=1.0, return_reduced=False, differentiable=False):
    """The steady states the rows of y0 ([B, N] or [B, 1, N] float32 on the device) relax to.  A gene moves in row b if
    relu(g) > 0 and it is not in row b's held set; `clamp` has the meaning and the forms it has in `odeint` (up to four genes
    per row, -1 / () for none).  Every other gene keeps its y0 value to the bit; the module is never modified.
    Per row: rho = max |r| over the moving genes, r = Wa h(y) - y; the row is done when rho <= tol, else it takes the
    linearly implicit step of m = tau g+ / (1 + tau g+); the step is accepted if the new rho' is finite and rho' <= 2 rho,
    and then tau <- tau min(10, max(2, rho / rho')); else y stays and tau <- tau / 4.  A row that is done is frozen.
    tau0 = float("inf") is plain Newton.  All max_iter passes are issued without a host synchronisation.
    Returns SteadyStates(y [B, N], residual [B] (rho of y), iterations [B] int32 (steps tried), status [B] int32 -- 0
    converged, 1 max_iter reached, 2 a singular or non-finite I - S --, tau [B], reduced): device tensors; reduced is S
    [B, 2H, 2H] with m = 1 on the moving genes at the result where return_reduced, else None.
    differentiable=True: the same iteration and the same values, but `y` carries a gradient to y0 and to the six parameter
    tensors of the module (the other fields stay plain tensors): the implicit adjoint of the fixed point (section 8q), one
    transposed 2H x 2H solve per row, no time integration.  The gradient of g is exactly 0 (a fixed point does not depend on
    the size of a positive multiplier), the gradient of y0 is exactly 0 on the genes that move (the attractor does not depend
    on where in its basin the row started) and dL/d(the level the gene is held at) on the others.  Only a converged row is a
    fixed point: MASK THE LOSS with `status == 0`.  A row that is not converged, or whose transposed system is singular (a
    bifurcation), contributes exact zeros to every gradient whatever the loss says; `last_backward_info()` tells which.
    The backward pass does not synchronise.  Once differentiable: no double backward; not for `GraphedStep` capture;
    `knockout_steady_states` stays without a gradient."""
    _check_control("steady_states", tol, max_iter, tau0)
    if differentiable:
        tensors = params_of(odenet)
        with torch.no_grad():
            p, y, free, gpos = _setup("steady_states", odenet, y0, clamp)
        y, rho, its, status, tau = _SteadyFn.apply(y0, (p, y, free, gpos, tol, max_iter, tau0), *tensors)
        with torch.no_grad():
            reduced = engine.reduced_jacobian(p, y.detach(), free.to(torch.float32))[0] if return_reduced else None
        return SteadyStates(y, rho, its, status, tau, reduced)
    with torch.no_grad():
        p, y, free, gpos = _setup("steady_states", odenet, y0, clamp)
        y, rho, its, status, tau = _relax(p, y, free, gpos, tol, max_iter, tau0)
        reduced = engine.reduced_jacobian(p, y, free.to(torch.float32))[0] if return_reduced else None
    return SteadyStates(y, rho, its, status, tau, reduced)


def knockout_steady_states(odenet, y0, genes, value=0.0, rows_per_call=256, **steady_kw):
    """Where does the system settle when gene g is HELD at `value`?  The unperturbed steady states of y0 are solved once;
    every knockout starts from them with gene genes[k] set to value[k] (a scalar or one level per gene) and held, and the
    K B rows go through `steady_states` in blocks of `rows_per_call` rows (a row's bits do not depend on its block).
    steady_kw: tol, max_iter, tau0 of `steady_states`.
    Returns KnockoutSteadyStates(genes, base, knockouts, shift [K, N], magnitude [K, N]): base the SteadyStates of y0,
    knockouts the SteadyStates of the K B rows (row k B + b), shift[k, n] the mean over the states of the settled level of
    target n under knockout k minus its unperturbed one, magnitude the mean of the absolute difference -- the shapes of
    `KnockoutEffects`' per-gene outputs, for `consolidate_gene_scores` as they are."""
    name = "knockout_steady_states"
    tensors = params_of(odenet)
    N = tensors[0].shape[1]
    if set(steady_kw) - {"tol", "max_iter", "tau0"}:
        raise TypeError("%s: unexpected arguments %s" % (name, sorted(set(steady_kw) - {"tol", "max_iter", "tau0"})))
    genes = engine.int_list(name, genes)
    engine.check_genes(name, genes, N)
    if not genes:
        raise ValueError("%s: no gene to hold" % name)
    values = engine.gene_values(name, value, len(genes))
    if isinstance(rows_per_call, bool) or not hasattr(rows_per_call, "__index__") or int(rows_per_call) < 1:
        raise ValueError("%s: rows_per_call must be a positive integer" % name)
    y2 = _rows(name, y0, N)
    B, K = y2.shape[0], len(genes)
    base = steady_states(odenet, y2, **steady_kw)
    with torch.no_grad():
        start = base.y.unsqueeze(0).repeat(K, 1, 1)
        for k, (gene, v) in enumerate(zip(genes, values)):
            start[k, :, gene] = v
        start = start.reshape(K * B, N)
        clamp = [(gene,) for gene in genes for _ in range(B)]
        step = min(int(rows_per_call), MAX_ROWS)
        parts = [steady_states(odenet, start[r0:r0 + step], clamp=clamp[r0:r0 + step], **steady_kw)[:5]
                 for r0 in range(0, K * B, step)]
        ko = SteadyStates(*(torch.cat(c) for c in zip(*parts)), None)
        d = ko.y.reshape(K, B, N) - base.y.unsqueeze(0)
        shift, magnitude = d.mean(dim=1), d.abs().mean(dim=1)
    return KnockoutSteadyStates(genes, base, ko, shift, magnitude)


def _response_args(name, N, regulators, input, reduce, rows_bytes=1):
    """the host checks `steady_state_response` and its reference share -> the regulators as a list"""
    if input not in ("level", "production"):
        raise ValueError('%s: input must be "level" or "production", got %r' % (name, input))
    if reduce not in ("mean_abs", "mean"):
        raise ValueError('%s: reduce must be "mean_abs" or "mean", got %r' % (name, reduce))
    if isinstance(rows_bytes, bool) or not hasattr(rows_bytes, "__index__") or int(rows_bytes) < 1:
        raise ValueError("%s: rows_bytes must be a positive integer" % name)
    regs = list(range(N)) if regulators is None else engine.int_list(name, regulators, "regulators")
    engine.check_genes(name, regs, N)
    if not regs:
        raise ValueError("%s: no regulator" % name)
    return regs


def _response_status(name, status, B):
    if status is None:
        return None
    if not torch.is_tensor(status):
        status = torch.as_tensor(np.asarray(status))
    if tuple(status.shape) != (B,) or status.is_floating_point() or status.is_complex():
        raise ValueError("%s: status must be [%d] integers, got %s %s" % (name, B, status.dtype, tuple(status.shape)))
    return status


def _response_scores(response, regs, N, xp):
    """mean of |response[i, j]| over the targets j != regulators[i]"""
    mag = xp.abs(response)
    at = xp.arange(len(regs))
    own = mag[at, regs if xp is np else torch.as_tensor(regs, device=response.device)]
    return (mag.sum(1) - own) / max(N - 1, 1)


def steady_state_response(odenet, y, clamp=None, regulators=None, input="level", reduce="mean_abs", status=None,
                          rows_bytes=256 << 20):
    """If gene i moves, where do all the other genes settle?  The network of total effects at the states y ([B, N] or
    [B, 1, N] float32 on the device, normally `steady_states(...).y`), every indirect path followed to the end (section 8r):
    on the moving genes r(y) + u = 0, so R = dy*/du = M + M Wa Z C M with Z = (I - S)^-1 -- all N answers of a state from one
    2H x 2H factorisation.  `clamp` as in `steady_states`; `regulators`: the K genes whose input moves (default all N).
    input="production": response[i, j] reduces R_b[j, regulators[i]], the shift of target j per unit of extra production of
    the regulator (exactly 0 for a regulator that does not move in row b).  input="level": the regulator is held and its
    LEVEL moves, R_b[j, i] / R_b[i, i]: exactly 1 at j = i, and for a regulator the row already holds the quantity
    `y0.grad[b, i]` of `steady_states(differentiable=True)` carries.  reduce: the mean over the used states of the entries
    ("mean") or of their absolute values ("mean_abs").  A row is left out -- it contributes exact zeros and the mean divides
    by the rest, counted on the device -- where I - S_b is singular or not finite, where `status` ([B] integers, e.g.
    `SteadyStates.status`) is not 0, and, for one regulator only, where its divisor d_bi = 1 + m_bi Wa[i, :] x_bi is 0 or
    not finite.  A target that moves in no used row is exactly 0 off the diagonal.
    Returns SteadyResponse(regulators, response [K, N] (regulator -> target), scores [K] (the mean of |response[i, j]| over
    j != regulators[i]; for `consolidate_gene_scores`), info [B] int32: 0 the row was used, -2 (`NOT_CONVERGED`) its status
    was not 0, else phx_steady_solve's code of I - S_b).  Device tensors; nothing is read back.  The regulators are walked in
    blocks whose factors [B, 2H, K_block] stay under `rows_bytes`; a block's rows have the bits of the full result."""
    name = "steady_state_response"
    tensors = params_of(odenet)
    N = tensors[0].shape[1]
    regs = _response_args(name, N, regulators, input, reduce, rows_bytes)
    y2 = _rows(name, y, N)
    B, K = y2.shape[0], len(regs)
    status = _response_status(name, status, B)
    with torch.no_grad():
        p, y2, free, _ = _setup(name, odenet, y2, clamp)
        dev = y2.device
        m = free.to(torch.float32)
        step = max(1, _block_rows(p) // 2)           # the inverse holds 2 (2H)^2 doubles per row
        parts = []
        for b0 in range(0, B, step):
            S, _w, hid = engine.reduced_jacobian(p, y2[b0:b0 + step], m[b0:b0 + step])
            parts.append((hid,) + engine.steady_inverse(S))
        hid, Z, info = (torch.cat(c) for c in zip(*parts)) if len(parts) > 1 else parts[0]
        if status is not None:
            info = torch.where(status.to(dev) != 0, NOT_CONVERGED, info).to(torch.int32)
        genes = torch.tensor(regs, dtype=torch.int32, device=dev)
        block = max(1, int(rows_bytes) // (B * 2 * p.H * 4))
        if block >= 64:
            block = block // 64 * 64                 # whole tiles of the hot kernel
        response = torch.empty((K, N), dtype=torch.float32, device=dev)
        for k0 in range(0, K, block):
            X, use = engine.steady_response_factors(p, y2, m, hid, Z, info, genes[k0:k0 + block], input)
            engine.steady_response(p, m, X, use, genes[k0:k0 + block], input, reduce == "mean_abs", response[k0:k0 + block])
        scores = _response_scores(response, regs, N, torch)
    return SteadyResponse(regs, response, scores, info)


# --------------------------------------------------------------------------------------------- the reference, no GPU
def _np_params(params, dtype):
    if isinstance(params, dict):
        t = [np.asarray(params[k]) for k in ("Ws", "bs", "Wp", "bp", "Wa", "g")]
    else:
        t = [x.detach().cpu().numpy() for x in params_of(params)]
    ws, bs, wp, bp, wa, g = (np.asarray(x, dtype) for x in t)
    return ws, bs, wp, bp, wa, g.reshape(-1)


def _np_parts(ws, bs, wp, bp, y):
    s = y - y.dtype.type(0.5)
    d = 1 + np.abs(s)
    a = s / d
    l = np.log1p(a)
    da = 1 / (d * d)
    dl = da / (1 + a)
    with np.errstate(over="ignore"):
        v = np.exp(l @ wp.T + bp)
    return a, l, da, dl, a @ ws.T + bs, v


def steady_states_reference(params, y0, clamp=None, tol=1e-5, max_iter=50, tau0=1.0, dtype=np.float64):
    """`steady_states` in numpy with a dense solve and no GPU: the same iteration, the same control, the arithmetic in `dtype`
    (the 2H x 2H solve in float64 either way).  params: a PHOENIX ODENet (on any device) or a dict of arrays Ws [H, N], bs,
    Wp, bp, Wa [N, 2H], g [N]; y0 [B, N].  Returns SteadyStates of numpy arrays; reduced is S [B, 2H, 2H] with m = 1 on the
    moving genes at the result."""
    _check_control("steady_states_reference", tol, max_iter, tau0)
    dt = np.dtype(dtype).type
    ws, bs, wp, bp, wa, g = _np_params(params, dt)
    H, N = ws.shape
    y = np.array(y0, dtype=dt).reshape(-1, N)
    B = y.shape[0]
    sets = _held_sets("steady_states_reference", clamp, B, N)
    free = np.repeat((g > 0)[None, :], B, axis=0)
    for b, s in enumerate(sets):
        free[b, list(s)] = False
    gf = np.where(free, np.maximum(g, 0)[None, :], 0).astype(dt)

    def state(y):
        a, l, da, dl, u, v = _np_parts(ws, bs, wp, bp, y)
        r = np.concatenate([u, v], axis=1) @ wa.T - y
        with np.errstate(invalid="ignore"):
            rho = np.where(free, np.abs(r), 0).max(axis=1)
        return r, rho, (da, dl, v)

    def C_of(b, d):
        da, dl, v = d
        return np.concatenate([ws * da[b][None, :], v[b][:, None] * wp * dl[b][None, :]], axis=0)

    r, rho, d = state(y)
    tau = np.full(B, tau0, dt)
    status = np.where(rho <= tol, CONVERGED, MAX_ITER).astype(np.int32)
    its = np.zeros(B, np.int32)
    eye = np.eye(2 * H)
    for _ in range(int(max_iter)):
        active = status == MAX_ITER
        if not active.any():
            break
        yc = y.copy()
        bad = np.zeros(B, bool)
        with np.errstate(all="ignore"):
            tg = tau[:, None] * gf
            m = np.where(free, np.where(np.isinf(tg), dt(1), tg / (1 + tg)), dt(0)).astype(dt)
            for b in np.nonzero(active)[0]:
                C = C_of(b, d)
                S = (C * m[b][None, :]) @ wa
                w = C @ (m[b] * np.where(free[b], r[b], 0))
                A = eye - S.astype(np.float64)
                try:
                    if not np.all(np.isfinite(A)):
                        raise np.linalg.LinAlgError
                    x = np.linalg.solve(A, w.astype(np.float64))
                    if not np.all(np.isfinite(x)):
                        raise np.linalg.LinAlgError
                except np.linalg.LinAlgError:
                    bad[b] = True
                    continue
                yc[b] = np.where(free[b], y[b] + m[b] * (r[b] + x.astype(dt) @ wa.T), y[b])
            rc, rhoc, dc = state(yc)
            ok = active & ~bad & np.isfinite(rhoc) & (rhoc <= 2 * rho)
            rejected = active & ~bad & ~ok
            grow = np.clip(rho / np.where(rhoc > 0, rhoc, dt(1e-300) if dt is np.float64 else dt(1e-45)), 2, 10).astype(dt)
            tau = np.where(ok, tau * grow, np.where(rejected, tau / 4, tau)).astype(dt)
        y[ok], r[ok], rho[ok] = yc[ok], rc[ok], rhoc[ok]
        for old, new in zip(d, dc):
            old[ok] = new[ok]
        its += active
        status = np.where(bad, SINGULAR, np.where(ok & (rhoc <= tol), CONVERGED, status)).astype(np.int32)
    reduced = np.stack([(C_of(b, d) * free[b][None, :].astype(dt)) @ wa for b in range(B)])
    return SteadyStates(y, rho, its, status, tau, reduced)


def steady_states_adjoint_reference(params, y, gy, clamp=None, status=None, dtype=np.float64):
    """The gradients `steady_states(differentiable=True)` returns, in numpy and without a GPU: the formulas of section 8q
    at the steady states y [B, N] for the cotangents gy [B, N] = dL/dy, the arithmetic in `dtype` (the transposed 2H x 2H
    solve in float64 either way).  params, clamp as in `steady_states_reference`; status [B] (optional): a row whose
    status is not 0 contributes exact zeros.  Returns SteadyAdjoint(y0 [B, N], Ws [H, N], bs, Wp, bp, Wa [N, 2H], g [N]
    (zeros), lam [B, N], q [B, 2H], info [B] int32 -- 0 used, -2 status != 0, 1 a singular transposed system, -1 a
    non-finite solution)."""
    dt = np.dtype(dtype).type
    ws, bs, wp, bp, wa, g = _np_params(params, dt)
    H, N = ws.shape
    y = np.array(y, dtype=dt).reshape(-1, N)
    gy = np.array(gy, dtype=dt).reshape(-1, N)
    B = y.shape[0]
    if gy.shape != y.shape:
        raise ValueError("steady_states_adjoint_reference: y and gy must have one shape")
    sets = _held_sets("steady_states_adjoint_reference", clamp, B, N)
    free = np.repeat((g > 0)[None, :], B, axis=0)
    for b, s in enumerate(sets):
        free[b, list(s)] = False
    info = np.zeros(B, np.int32)
    if status is not None:
        info[np.asarray(status).reshape(B) != 0] = NOT_CONVERGED
    with np.errstate(all="ignore"):
        a, l, da, dl, u, v = _np_parts(ws, bs, wp, bp, y)
    q, lam, gy0 = np.zeros((B, 2 * H), dt), np.zeros((B, N), dt), np.zeros((B, N), dt)
    eye = np.eye(2 * H)
    for b in np.nonzero(info == 0)[0]:
        C = np.concatenate([ws * da[b][None, :], v[b][:, None] * wp * dl[b][None, :]], axis=0)
        S = (C * free[b][None, :].astype(dt)) @ wa
        rhs = wa.T @ np.where(free[b], gy[b], dt(0))
        A = eye - S.T.astype(np.float64)
        try:
            if not np.all(np.isfinite(A)):
                raise np.linalg.LinAlgError
            x = np.linalg.solve(A, rhs.astype(np.float64))
        except np.linalg.LinAlgError:
            info[b] = 1
            continue
        if not np.all(np.isfinite(x)):
            info[b] = -1
            continue
        q[b] = x.astype(dt)
        w = gy[b] + q[b] @ C
        lam[b] = np.where(free[b], w, dt(0))
        gy0[b] = np.where(free[b], dt(0), w)
    used = (info == 0)[:, None]
    hid = np.where(used, np.concatenate([u, v], axis=1), dt(0))
    qv = q[:, H:] * hid[:, H:]
    return SteadyAdjoint(gy0, q[:, :H].T @ np.where(used, a, dt(0)), q[:, :H].sum(axis=0), qv.T @ np.where(used, l, dt(0)),
                         qv.sum(axis=0), lam.T @ hid, np.zeros(N, dt), lam, q, info)


def steady_state_response_reference(params, y, clamp=None, regulators=None, input="level", reduce="mean_abs", status=None,
                                    dtype=np.float64):
    """`steady_state_response` in numpy without a GPU: the same formulas at the states y [B, N], the arithmetic in `dtype`
    (the 2H x 2H inverse in float64 either way).  params, clamp as in `steady_states_reference`.  Returns SteadyResponse of
    numpy arrays; info is 0, -2 (status != 0), 1 (a singular I - S_b, whatever its column) or -1 (a non-finite inverse)."""
    name = "steady_state_response_reference"
    dt = np.dtype(dtype).type
    ws, bs, wp, bp, wa, g = _np_params(params, dt)
    H, N = ws.shape
    regs = _response_args(name, N, regulators, input, reduce)
    y = np.array(y, dtype=dt).reshape(-1, N)
    B, K = y.shape[0], len(regs)
    sets = _held_sets(name, clamp, B, N)
    free = np.repeat((g > 0)[None, :], B, axis=0)
    for b, s in enumerate(sets):
        free[b, list(s)] = False
    info = np.zeros(B, np.int32)
    if status is not None:
        info[np.asarray(status).reshape(B) != 0] = NOT_CONVERGED
    with np.errstate(all="ignore"):
        a, l, da, dl, u, v = _np_parts(ws, bs, wp, bp, y)
    acc, cnt = np.zeros((K, N), dt), np.zeros(K, dt)
    eye, at = np.eye(2 * H), np.arange(K)
    for b in np.nonzero(info == 0)[0]:
        mb = free[b].astype(dt)
        C = np.concatenate([ws * da[b][None, :], v[b][:, None] * wp * dl[b][None, :]], axis=0)
        A = eye - ((C * mb[None, :]) @ wa).astype(np.float64)
        try:
            if not np.all(np.isfinite(A)):
                raise np.linalg.LinAlgError
            Z = np.linalg.inv(A)
        except np.linalg.LinAlgError:
            info[b] = 1
            continue
        if not np.all(np.isfinite(Z)):
            info[b] = -1
            continue
        with np.errstate(all="ignore"):
            X = Z.astype(dt) @ C[:, regs]                                # [2H, K]
            d = 1 + mb[regs] * np.einsum("kc,ck->k", wa[regs], X)
            ok = np.isfinite(d) & (d != 0)
            T = mb[:, None] * (wa @ X)                                   # [N, K]: target j, regulator k
            if input == "production":
                R = T * mb[regs][None, :]
                R[regs, at] += mb[regs]
            else:
                R = T / np.where(ok, d, 1)[None, :]
                R[regs, at] = 0
            R[:, ~ok] = 0
        acc += np.abs(R.T) if reduce == "mean_abs" else R.T
        cnt += ok
    response = acc / np.where(cnt > 0, cnt, 1)[:, None]
    if input == "level":
        response[at, regs] = cnt > 0
    return SteadyResponse(regs, response, _response_scores(response, regs, N, np), info)
