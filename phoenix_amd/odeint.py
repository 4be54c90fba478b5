"""Drop-in `odeint` / `odeint_adjoint` for PHOENIX's ODENet on MI355X.

Mirrors the reference surface (vendored torchdiffeq 0.1.1):
    odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None)          _impl/odeint.py:30
    odeint_adjoint(func, y0, t, rtol, atol, method, options, adjoint_rtol, adjoint_atol,
                   adjoint_method, adjoint_options, adjoint_params)                 _impl/adjoint.py:165
Same argument meaning, output shape `[len(t), *y0.shape]`, default method 'dopri5', the same
exceptions (ValueError for an unknown method, AssertionError for the solver asserts).

Extension (what the reference's training loop *means*, train_insilico.py:128-130): `t` may be 2-D
`[B, T]` -- one time grid per sample of `y0 [B, 1, N]` -- which integrates all B samples in ONE launch
with an independent step controller per sample (`odeint_per_sample` is the explicit spelling)."""
import math
import warnings

import torch

from . import _lib, engine, generic
from .odenet import params_of

# torchdiffeq's registry (odeint.py:14-27); the engine implements the ones PHOENIX's configs use.
SOLVERS = ("dopri8", "dopri5", "bosh3", "adaptive_heun", "euler", "midpoint", "rk4", "explicit_adams",
           "implicit_adams", "fixed_adams")
_ENGINE_METHODS = ("dopri5", "euler", "midpoint", "rk4")
_FIXED_GRID_METHODS = ("euler", "midpoint", "rk4")
_KNOWN_UNSUPPORTED_OPTIONS = ("grid_constructor", "grid_points", "eps", "first_step", "safety",
                              "ifactor", "dfactor", "norm", "dtype")


def _step_size(value):
    """options["step_size"] as a float: a Python number or a 0-d tensor, positive and finite"""
    if torch.is_tensor(value):
        if value.numel() != 1:
            raise ValueError("phoenix_amd: step_size must be a number or a 0-d tensor")
        value = value.item()
    try:
        h = float(value)
    except (TypeError, ValueError):
        raise ValueError("phoenix_amd: step_size must be a positive finite number, got %r" % (value,)) from None
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError("phoenix_amd: step_size must be a positive finite number, got %r" % (value,))
    return h


def _check_inputs(func, y0, t, rtol, atol, method, options):
    """misc.py:165-241, restricted to what the engine supports.  options["step_size"] comes back validated, as a float,
    for the fixed-grid methods; dopri5 drops it with the reference's warning (misc.py:204-206)."""
    if not torch.is_tensor(y0):
        raise NotImplementedError("phoenix_amd: tuple states are not supported (PHOENIX passes a single tensor)")
    if not torch.is_floating_point(y0):
        raise TypeError("`y0` must be a floating point Tensor but is a {}".format(y0.type()))
    if y0.dtype != torch.float32:
        raise NotImplementedError("phoenix_amd: the engine computes in float32 like the reference's configs; "
                                  "got y0 dtype %s" % y0.dtype)
    options = {} if options is None else dict(options)
    if method is None:
        method = "dopri5"
    if method not in SOLVERS:
        raise ValueError('Invalid method "{}". Must be one of {}'.format(
            method, '{"' + '", "'.join(SOLVERS) + '"}.'))
    if method not in _ENGINE_METHODS:
        raise NotImplementedError("phoenix_amd: method '%s' is registered in torchdiffeq but not on PHOENIX's "
                                  "path (configs use dopri5; rk4/euler/midpoint are implemented)" % method)
    assert torch.is_tensor(t), "t must be a torch.Tensor"
    assert t.ndimension() in (1, 2), "t must be one dimensional"
    if not torch.is_floating_point(t):
        raise TypeError("`t` must be a floating point Tensor but is a {}".format(t.type()))
    for k in list(options):
        if k in _KNOWN_UNSUPPORTED_OPTIONS:
            raise NotImplementedError("phoenix_amd: solver option '%s' is not supported by the fused stepper" % k)
        if k == "step_size" and method in _FIXED_GRID_METHODS:
            options[k] = _step_size(options[k])
        elif k not in ("max_num_steps", "batch_control"):
            warnings.warn("phoenix_amd: Unexpected arguments {}".format({k: options.pop(k)}))
    if torch.is_tensor(rtol) or torch.is_tensor(atol):
        rtol, atol = float(rtol), float(atol)
    return y0, t, float(rtol), float(atol), method, options


def _is_odenet(func):
    try:
        params_of(func)
        return True
    except TypeError:
        return False


def _prepare(func, y0, t, options):
    ws, bs, wp, bp, wa, g = params_of(func)
    N = ws.shape[1]
    if y0.shape[-1] != N:
        raise ValueError("phoenix_amd: y0 last dimension %d != number of genes %d" % (y0.shape[-1], N))
    engine._require_gpu(y0, "y0")
    y2 = y0.reshape(-1, N)
    B = y2.shape[0]
    if t.device != y0.device:
        warnings.warn("t is not on the same device as y0. Coercing to y0.device.")   # misc.py:232-235
    if t.dtype == torch.float32:     # the engine reads a float32 grid as it is (time arithmetic stays fp64 inside)
        t_is_f32 = 2
        t64 = t.detach().to(device=y0.device).contiguous()
    else:
        t_is_f32 = 0
        t64 = t.detach().to(device=y0.device, dtype=torch.float64).contiguous()
    per_sample = t.ndimension() == 2
    if per_sample and t.shape[0] != B:
        raise ValueError("phoenix_amd: per-sample t must be [B, T] with B = %d trajectories" % B)
    ctl = options.get("batch_control", "per_trajectory" if per_sample else "shared")
    if ctl not in ("shared", "per_trajectory"):
        raise ValueError("batch_control must be 'shared' or 'per_trajectory'")
    if per_sample and ctl == "shared":
        raise ValueError("per-sample time grids need batch_control='per_trajectory'")
    control = _lib.CTRL_SHARED if ctl == "shared" else _lib.CTRL_PER_TRAJECTORY
    return (ws, bs, wp, bp, wa, g), y2, t64, B, N, per_sample, t_is_f32, control


def _out_shape(sol, y0, per_sample):
    # [T, B, N] -> [T, *y0.shape]
    return sol.reshape((sol.shape[0],) + tuple(y0.shape))


class _RowClamp:
    """The held sets of one odeint / odeint_adjoint call, one per trajectory row: `sets` (B sorted tuples, at least one
    of them non-empty), the rows grouped by identical set in sorted order of the sets (the grouped path solves them in
    this order), and -- set by the forward solve where the per-row kernels serve the call -- the device list they read."""

    def __init__(self, sets):
        self.sets = sets
        groups = {}
        for b, s in enumerate(sets):
            groups.setdefault(s, []).append(b)
        self.groups = sorted(groups.items())
        self.dev = None          # int32 [B, width], shorter sets padded with -1: the kernel path
        self.bp_steps = []       # grouped path, backpropagation through the steps: require_backprop's answer per group

    def device_list(self, device):
        width = max(1, max(len(s) for s in self.sets))
        return torch.tensor([list(s) + [-1] * (width - len(s)) for s in self.sets], dtype=torch.int32).to(device)


def _row_clamp(who, func, y0, t, options, clamp):
    """`clamp` of odeint / odeint_adjoint / odeint_per_sample as a _RowClamp, or None where every set is empty (the call
    then runs the unclamped entry points unchanged).  `_clamp_list`'s checks with one entry per trajectory row, on the
    host, before anything is launched or asked of the device."""
    if clamp is None:
        return None
    N = params_of(func)[0].shape[1]
    if y0.shape[-1] != N:
        raise ValueError("phoenix_amd: y0 last dimension %d != number of genes %d" % (y0.shape[-1], N))
    sets = _clamp_list(clamp, y0.numel() // N, N, who=who, unit="row")
    if not any(sets):
        return None
    ctl = options.get("batch_control", "per_trajectory" if t.ndimension() == 2 else "shared")
    if ctl != "per_trajectory":
        raise ValueError("%s: a clamp per trajectory row needs per-trajectory step control (t [B, T], or options="
                         "{'batch_control': 'per_trajectory'}); under one shared controller per call use "
                         "odeint_calls(..., clamp=...), whose clamp is per call" % who)
    return _RowClamp(sets)


def _group_params(params, held):
    """engine parameters of the model a row with the held set `held` is defined by: g zeroed on the set, in a clone --
    the caller's module is never modified"""
    if not held:
        return engine.params_cached(*params)
    ws, bs, wp, bp, wa, g = params
    gk = g.detach().clone()
    gk.reshape(-1)[list(held)] = 0.0
    return engine.Params(ws, bs, wp, bp, wa, gk)


def _rows_of(rows, t64, per_sample, device):
    idx = torch.tensor(rows, dtype=torch.long, device=device)
    return idx, (t64.index_select(0, idx) if per_sample else t64)


def _clamped_rows_forward(params, y2, t64, cfg, clamp, adjoint, stats=None):
    """forward solve of a per-row clamped call -> sol [T,B,N], status (None: already checked), nfe, nsteps, Params (None
    on the grouped path).  One launch of the per-row kernels (engine.solve_forward_clamped_rows) where they serve the
    call -- and, with `adjoint`, its backward solve too --; else the grouped path: the rows of every distinct set, in
    sorted order of the sets, through the ordinary entry points on `_group_params`, status checked per group."""
    (method, control, rtol, atol, per_sample, t_is_f32, max_steps, adj, _defer, steps) = cfg
    N, H, B, T = params[0].shape[1], params[0].shape[0], y2.shape[0], t64.shape[-1]
    backprop = adjoint and adj[3] and adj[0] in _FIXED_GRID_METHODS
    y2 = y2.detach().contiguous()
    if (engine.clamped_rows_plan_exists(_lib.OP_ODEINT, N, H, B, T, method) and
            (not adjoint or engine.clamped_rows_plan_exists(_lib.OP_ADJOINT, N, H, B, T, adj[0]))):
        p = engine.params_cached(*params)
        clamp.dev = clamp.device_list(y2.device)
        sol, status, nfe, nsteps = engine.solve_forward_clamped_rows(p, y2, t64, clamp.dev, rtol, atol, per_sample,
                                                                     t_is_f32, max_steps, stats=stats)
        return sol, status, nfe, nsteps, p
    sol = torch.empty((T, B, N), dtype=torch.float32, device=y2.device)
    nfe = torch.empty(B, dtype=torch.int32, device=y2.device)
    nsteps = torch.empty(B, dtype=torch.int32, device=y2.device)
    clamp.bp_steps = []
    for held, rows in clamp.groups:
        idx, tg = _rows_of(rows, t64, per_sample, y2.device)
        p = _group_params(params, held)
        if backprop:      # refused here, at the call, like the unclamped solve
            clamp.bp_steps.append(engine.require_backprop(N, H, len(rows), T, method, tg, steps[0]))
        if steps[0] or (adjoint and steps[1]):
            if steps[0]:
                engine.require_stepped_kernels(p, len(rows), T, method, backward=False)
            if adjoint and steps[1] and not backprop:
                engine.require_stepped_kernels(p, len(rows), T, adj[0], forward=False)
        one, status, nf, ns = engine.solve_forward(p, y2.index_select(0, idx), tg, method, control, rtol, atol, per_sample,
                                                   t_is_f32, max_steps, step_size=steps[0])
        engine.raise_for_status(status)
        sol[:, idx] = one
        nfe[idx] = nf
        nsteps[idx] = ns
    return sol, None, nfe, nsteps, None


def _clamped_rows_backward(params, t64, sol, grad_sol, cfg, clamp, p, need_p, stats=None):
    """backward solve of a per-row clamped call -> adj_y0 [B,N], Grads or None, status (None: checked per group).  The
    kernel path where the forward took it (clamp.dev); else group by group in the forward's order, the parameter
    gradients accumulated into ONE Grads in that order and adj_y0 scattered back to the caller's rows."""
    (method, control, _rtol, _atol, per_sample, t_is_f32, max_steps, adj, _defer, steps) = cfg
    a_method, a_rtol, a_atol, via_odeint = adj
    grad_sol = grad_sol.contiguous()
    if clamp.dev is not None:
        adj_y0, grads, status, _nfe, _ns = engine.solve_adjoint_clamped_rows(
            p, t64, sol, grad_sol, clamp.dev, a_rtol, a_atol, per_sample, t_is_f32, want_grads=need_p,
            max_num_steps=max_steps, stats=stats)
        return adj_y0, grads, status
    T, B, N = sol.shape
    adj_y0 = torch.empty((B, N), dtype=torch.float32, device=sol.device)
    grads = None
    for i, (held, rows) in enumerate(clamp.groups):
        idx, tg = _rows_of(rows, t64, per_sample, sol.device)
        pg = _group_params(params, held)
        if need_p and grads is None:
            grads = pg.new_grads()      # the first group writes it (overwrite), the later ones add
        ys, gs = sol.index_select(1, idx), grad_sol.index_select(1, idx)
        if via_odeint and a_method in _FIXED_GRID_METHODS:
            a, _g, status, _nfe, _ns = engine.solve_backprop(
                pg, tg, ys, gs, method, control, per_sample, t_is_f32, want_grads=need_p, max_num_steps=max_steps,
                step_size=steps[0], grid_steps=clamp.bp_steps[i], grads=grads)
        else:
            a, _g, status, _nfe, _ns = engine.solve_adjoint(
                pg, tg, ys, gs, a_method, control, a_rtol, a_atol, per_sample, t_is_f32, want_grads=need_p,
                max_num_steps=max_steps, step_size=steps[1], grads=grads)
        engine.raise_for_status(status)
        if grads is not None:
            grads.c.overwrite = 0
        adj_y0[idx] = a
    return adj_y0, grads, None


def _queue_status(stats):
    """the status read-back of a training step, raised from loss.backward() (see _OdeintAdjointFn.backward)"""
    if engine.status_mode() == "deferred":
        engine.defer_status(stats)      # checked at a later engine call, once the kernel has finished
    else:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(lambda: engine.raise_for_status(stats))
        except Exception:   # noqa: BLE001  (no running graph task: check right here)
            engine.raise_for_status(stats)


class _OdeintAdjointFn(torch.autograd.Function):
    """OdeintAdjointMethod (adjoint.py:9-162): forward = no-grad solve, saves (t, y, params);
    backward = reverse-time augmented solve on the engine.  clamp: a _RowClamp (held genes per trajectory row), carried
    from forward to backward with its device list."""

    @staticmethod
    def forward(ctx, y2, t64, cfg, ws, bs, wp, bp, wa, g, clamp=None):
        (method, control, rtol, atol, per_sample, t_is_f32, max_steps, adj, defer, steps) = cfg
        engine.check_pending_status()
        ctx.phx_clamp = clamp
        if clamp is not None:
            stats = torch.empty((3, 2 if defer else 1, y2.shape[0]), dtype=torch.int32, device=y2.device)
            ctx.set_materialize_grads(False)
            sol, status, nfe, _ns, p = _clamped_rows_forward((ws, bs, wp, bp, wa, g), y2, t64, cfg, clamp, True, stats[:, 0])
            # (the grouped path has checked every group; the kernel path defers like the unclamped solve below)
            ctx.phx_stats = stats if defer and status is not None else None
            if status is not None and not defer:
                engine.raise_for_status(status)
            ctx.cfg = cfg
            ctx.phx_params = p
            ctx.phx_versions = tuple(x._version for x in (ws, bs, wp, bp, wa, g))
            ctx.save_for_backward(t64, sol, ws, bs, wp, bp, wa, g)
            ctx.mark_non_differentiable(nfe)
            return sol, nfe
        # odeint(method=<fixed grid>) whose backward pass backpropagates through the steps: every shape that pass would
        # refuse is refused HERE, at the call, before anything is launched (H > 128, PHX_ENGINE=v0, a grid whose
        # checkpoints exceed engine.BACKPROP_MAX_CHECKPOINT_BYTES)
        backprop = adj[3] and adj[0] in _FIXED_GRID_METHODS
        ctx.phx_bp_steps = (engine.require_backprop(ws.shape[1], ws.shape[0], y2.shape[0], t64.shape[-1], method, t64, steps[0])
                            if backprop else 0)
        p = engine.params_cached(ws, bs, wp, bp, wa, g)
        if steps[0] or steps[1]:      # both solves of the step, or neither
            B, T = y2.shape[0], t64.shape[-1]
            if steps[0]:
                engine.require_stepped_kernels(p, B, T, method, backward=False)
            if steps[1] and defer and not backprop:    # (defer: a backward pass can come)
                engine.require_stepped_kernels(p, B, T, adj[0], forward=False)
        # one stats block for both launches of the step, [status | nfe | nsteps][launch: forward, backward][B]: the two
        # status rows are contiguous (one copy to the host), and nothing is zero-filled -- every solve kernel writes the
        # three entries of every trajectory of its launch
        stats = torch.empty((3, 2 if defer else 1, y2.shape[0]), dtype=torch.int32, device=y2.device)
        ctx.set_materialize_grads(False)      # no zero tensor for the (non-differentiable) nfe output in backward
        sol, status, nfe, nsteps = engine.solve_forward(p, y2.detach().contiguous(), t64, method, control, rtol,
                                                        atol, per_sample, t_is_f32, max_steps, stats=stats[:, 0],
                                                        step_size=steps[0])
        # The reference raises the solver's AssertionErrors synchronously.  When a backward pass is coming
        # (some input requires grad) the forward status is read together with the backward solve's status, in
        # ONE host<->device round trip per training step after both launches are queued: same exception (the
        # forward's first), raised from backward().  Outputs a failed forward never reached are NaN, which stops
        # the backward solve at once.  Without autograd (validation, analysis callers) the check is immediate.
        ctx.phx_stats = stats if defer else None
        ctx.phx_fwd_status = status if defer else None
        if ctx.phx_fwd_status is None:
            engine.raise_for_status(status)
        ctx.cfg = cfg
        ctx.phx_params = p   # engine-layout views (incl. the transposed Wa copy) reused by backward
        ctx.phx_versions = tuple(x._version for x in (ws, bs, wp, bp, wa, g))
        ctx.save_for_backward(t64, sol, ws, bs, wp, bp, wa, g)
        ctx.mark_non_differentiable(nfe)
        return sol, nfe

    @staticmethod
    def backward(ctx, grad_sol, _grad_nfe):
        t64, sol, ws, bs, wp, bp, wa, g = ctx.saved_tensors
        if grad_sol is None:
            grad_sol = torch.zeros_like(sol)
        (method, control, rtol, atol, per_sample, t_is_f32, max_steps, adj, _defer, steps) = ctx.cfg
        a_method, a_rtol, a_atol, via_odeint = adj
        p = ctx.phx_params
        if ctx.phx_versions != tuple(x._version for x in (ws, bs, wp, bp, wa, g)):
            p = engine.params_cached(ws, bs, wp, bp, wa, g)   # parameters were modified in place since forward
        need_p = any(ctx.needs_input_grad[3:9])
        bstats = None if ctx.phx_stats is None else ctx.phx_stats[:, 1]
        if ctx.phx_clamp is not None:
            adj_y0, grads, status = _clamped_rows_backward((ws, bs, wp, bp, wa, g), t64, sol, grad_sol, ctx.cfg,
                                                           ctx.phx_clamp, p, need_p, bstats)
            if status is not None:      # the kernel path: one read-back for both launches, as below
                _queue_status(status if ctx.phx_stats is None else ctx.phx_stats[0])
            gp = grads.as_reference_layout(g.shape) if need_p else (None,) * 6
            return (adj_y0, None, None) + tuple(gp) + (None,)
        if via_odeint and a_method in _FIXED_GRID_METHODS:
            # the reference's `odeint`: backpropagation through the solver's own steps (the discrete adjoint), not the
            # continuous adjoint below, from which it differs at O(1) for one unconverged step per interval
            adj_y0, grads, status, _nfe, _ns = engine.solve_backprop(
                p, t64, sol, grad_sol.contiguous(), method, control, per_sample, t_is_f32, want_grads=need_p,
                max_num_steps=max_steps, stats=bstats, step_size=steps[0], grid_steps=ctx.phx_bp_steps)
        else:
            adj_y0, grads, status, _nfe, _ns = engine.solve_adjoint(
                p, t64, sol, grad_sol.contiguous(), a_method, control, a_rtol, a_atol, per_sample, t_is_f32,
                want_grads=need_p, max_num_steps=max_steps, stats=bstats, step_size=steps[1])
        # The status read-back is the one host<->device round trip of a training step.  It is queued as an
        # end-of-backward callback of the autograd engine (the mechanism DDP finalises with): the exception still comes
        # out of loss.backward(), but the host returns the gradients and runs its accumulation nodes while the kernel
        # is still executing instead of after it.
        _queue_status(status if ctx.phx_stats is None else ctx.phx_stats[0])    # [2, B]: forward and backward status
        if need_p:
            gws, gbs, gwp, gbp, gwa, gg = grads.as_reference_layout(g.shape)
        else:
            gws = gbs = gwp = gbp = gwa = gg = None
        return adj_y0, None, None, gws, gbs, gwp, gbp, gwa, gg, None


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, return_stats=False, clamp=None):
    """odeint.py:30-74.  The reference's `odeint` returns an autograd-tracked solution (backpropagation through the
    solver's own operations).  For an ODENet:
      * nothing requires grad, autograd is off (validation, analysis callers), or `return_stats`: plain forward solve
        (`return_stats=True` is forward-only: its result carries no autograd history);
      * something requires grad, euler / midpoint / rk4 (one step per interval, or the steps of options["step_size"]):
        the result is differentiable by backpropagation through the fixed-grid steps -- the discrete adjoint, computed by
        one persistent kernel (phx_odeint_backprop_backward): the exact gradient of the numbers the forward pass
        produced, whatever the step, like the reference's.  `odeint_adjoint` stays the continuous adjoint, which differs
        from it at O(1) for one unconverged step per interval.  Under a step size the backward pass re-runs the forward
        grid and keeps the start state of every step (steps x B x N x 4 bytes).  A call whose backward pass could not be
        served raises RuntimeError HERE, not from backward(): hidden layers over H = 128, PHX_ENGINE=v0, a grid whose
        checkpoints exceed engine.BACKPROP_MAX_CHECKPOINT_BYTES.  Solver assertions of the forward solve
        (max_num_steps exceeded) are then raised with the backward's, from backward(), as for `odeint_adjoint`;
      * something requires grad, dopri5: the call is routed through `odeint_adjoint`; the continuous adjoint agrees with
        backpropagation through the converged solve to the solver tolerance (<= 2e-6 relative).
    Gradients with respect to `t` are not computed.
    clamp (one entry per trajectory ROW of y0; None: no gene is held): see `odeint_adjoint`.  Note that `odeint_calls`'
    clamp is per CALL (one shared controller, forward only); this one is per row and differentiable."""
    y0, t, rtol, atol, method, options = _check_inputs(func, y0, t, rtol, atol, method, options)
    if not _is_odenet(func):      # any other module: unfused torch stepper, differentiable by plain backpropagation
        if clamp is not None:
            raise NotImplementedError("phoenix_amd: odeint: clamp needs a PHOENIX ODENet")
        engine._require_gpu(y0, "y0")          # like every other entry point: no CPU compute path in this package
        assert t.ndimension() == 1 and not return_stats, "per-sample grids / solver statistics need a PHOENIX ODENet"
        return generic.odeint(func, y0, t, rtol, atol, method, options)
    if not return_stats and torch.is_grad_enabled() and (y0.requires_grad or any(x.requires_grad for x in params_of(func))):
        return odeint_adjoint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options, _via_odeint=True,
                              clamp=clamp, _who="odeint")
    held = _row_clamp("odeint", func, y0, t, options, clamp)
    params, y2, t64, B, N, per_sample, t_is_f32, control = _prepare(func, y0, t, options)
    engine.check_pending_status()
    if held is not None:
        cfg = (method, control, rtol, atol, per_sample, t_is_f32, int(options.get("max_num_steps", 0)), None, False,
               (options.get("step_size", 0.0), 0.0))
        sol, status, nfe, nsteps, _p = _clamped_rows_forward(params, y2, t64, cfg, held, False)
        if status is not None:
            engine.raise_for_status(status)
        out = _out_shape(sol, y0, per_sample)
        return (out, nfe, nsteps) if return_stats else out
    p = engine.params_cached(*params)
    sol, status, nfe, nsteps = engine.solve_forward(p, y2.detach().contiguous(), t64, method, control, rtol, atol,
                                                    per_sample, t_is_f32, int(options.get("max_num_steps", 0)),
                                                    step_size=options.get("step_size", 0.0))
    engine.raise_for_status(status)
    out = _out_shape(sol, y0, per_sample)
    return (out, nfe, nsteps) if return_stats else out


_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _clamp_list(clamp, K, N, who="odeint_calls", unit="call"):
    """`clamp` of odeint_calls as K sorted tuples of distinct genes in [0, N) -- the set each call holds, () for none --
    checked on the host before anything is launched.  Per call an int (-1: none) or a sequence of at most
    engine.CLAMP_MAX ints, or for all calls a 1-D / 2-D integer tensor, -1 entries being padding.
    who, unit: the caller and what an entry belongs to, for the messages (odeint / odeint_adjoint / odeint_per_sample
    hold a set per trajectory ROW: the same checks with K = the rows)."""
    if torch.is_tensor(clamp):
        if clamp.dim() not in (1, 2) or clamp.dtype not in _INT_DTYPES:
            raise TypeError("%s: clamp must be a 1-D or 2-D integer tensor or a sequence of ints / int sequences, "
                            "got %s %s" % (who, clamp.dtype, tuple(clamp.shape)))
        clamp = clamp.tolist()
    try:
        clamp = list(clamp)
    except TypeError:
        raise TypeError("%s: clamp must be a sequence of %d ints or int sequences" % (who, K)) from None
    sets = []
    for entry in clamp:
        if hasattr(entry, "tolist"):      # numpy and tensor scalars / rows
            entry = entry.tolist()
        genes = list(entry) if isinstance(entry, (list, tuple, range, set, frozenset)) else [entry]
        for g in genes:
            if isinstance(g, bool) or not hasattr(g, "__index__"):
                raise TypeError("%s: clamp entries must be integers, got %r" % (who, g))
        sets.append([int(g) for g in genes])
    if len(sets) != K:
        raise ValueError("%s: clamp names genes for %d %ss, there are %d" % (who, len(sets), unit, K))
    for genes in sets:
        for g in genes:
            if g < -1 or g >= N:
                raise ValueError("%s: clamp entry %d is not a gene of 0 .. %d (or -1: none)" % (who, g, N - 1))
        if len(genes) > engine.CLAMP_MAX:
            raise ValueError("%s: a clamp set of %d entries, a %s holds at most %d genes"
                             % (who, len(genes), unit, engine.CLAMP_MAX))
    return [tuple(sorted(set(g for g in genes if g >= 0))) for genes in sets]     # duplicates count once


def _clamped_block(func, y0s, t, rtol, atol, method, options, clamp):
    """`_calls_block` with call k's genes clamp[k] (one gene or a set of up to four; -1: none) held at their initial
    values: one launch of phx_odeint_clamped_sets where dopri5 plans the calls on the third-generation kernels, else the
    K calls one by one on a parameter set whose g is zeroed on the set -- the model the clamped call is defined by."""
    K = y0s.shape[0]
    clamp = _clamp_list(clamp, K, params_of(func)[0].shape[1])      # first: a bad list is refused whatever else holds
    grids = torch.is_tensor(t) and t.ndimension() == 2
    if grids and t.shape[0] != K:
        raise ValueError("odeint_calls: t must be [T] or [K, T] with K = %d calls, got %s" % (K, tuple(t.shape)))
    y0, t, rtol, atol, method, options = _check_inputs(func, y0s, t, rtol, atol, method, options)
    params, y2, t1, B, N, per_sample, t_is_f32, control = _prepare(func, y0, t[0] if grids else t, options)
    if per_sample or control != _lib.CTRL_SHARED:
        raise ValueError("odeint_calls: one shared time grid per call, batch_control='shared'")
    # the grid as K rows, in the dtype the engine reads (a 1-D grid is expanded to K equal rows)
    tK = t.detach().to(device=y0.device, dtype=t1.dtype)
    tK = (tK if grids else tK.reshape(1, -1).expand(K, -1)).contiguous()
    T = tK.shape[-1]
    max_steps = int(options.get("max_num_steps", 0))
    engine.check_pending_status()
    if method == "dopri5" and engine.clamped_plan_exists(N, params[0].shape[0], B, T, K):
        p = engine.params_cached(*params)
        width = max(1, max(len(c) for c in clamp))      # the list as [K, width], shorter sets padded with -1
        genes = torch.tensor([list(c) + [-1] * (width - len(c)) for c in clamp], dtype=torch.int32).to(y0.device)
        sol, status, _, _ = engine.solve_forward_clamped(p, y2.detach().contiguous(), tK, genes, rtol, atol, t_is_f32,
                                                         max_steps)
        engine.raise_for_status(status)
        return sol
    # one by one: the caller's module is never modified, the zeroed multiplier lives in a clone
    ws, bs, wp, bp, wa, g = params
    Bc = B // K
    y2 = y2.detach().contiguous()
    block = torch.empty((T, K, Bc, N), dtype=torch.float32, device=y0.device)
    with torch.no_grad():
        for k in range(K):
            if not clamp[k]:
                p = engine.params_cached(*params)
            else:
                gk = g.detach().clone()
                gk.reshape(-1)[list(clamp[k])] = 0.0
                p = engine.Params(ws, bs, wp, bp, wa, gk)
            one, status, _, _ = engine.solve_forward(p, y2[k * Bc:(k + 1) * Bc], tK[k], method, control, rtol, atol, False,
                                                     t_is_f32, max_steps, step_size=options.get("step_size", 0.0))
            engine.raise_for_status(status)
            block[:, k] = one
    return block.reshape(T, K * Bc, N)


def _calls_block(func, y0s, t, rtol=1e-7, atol=1e-9, method=None, options=None, clamp=None):
    """the solves of `odeint_calls` as the engine's own output block: [T, K*B, N], call k in rows k*B .. (k+1)*B - 1 of
    every output time (B = trajectories of one call).  One batched launch where the plan exists; else the K calls one by
    one, copied into the same layout.  clamp: `_clamped_block`."""
    if clamp is not None:
        return _clamped_block(func, y0s, t, rtol, atol, method, options, clamp)
    K = y0s.shape[0]
    grids = torch.is_tensor(t) and t.ndimension() == 2
    if grids and t.shape[0] != K:
        raise ValueError("odeint_calls: t must be [T] or [K, T] with K = %d calls, got %s" % (K, tuple(t.shape)))
    t_of = (lambda k: t[k]) if grids else (lambda k: t)

    def one_by_one():
        block = None
        with torch.no_grad():     # forward-only by contract, like the batched launch below
            for k in range(K):
                one = odeint(func, y0s[k], t_of(k), rtol, atol, method, options)
                one = one.reshape(one.shape[0], -1, one.shape[-1])
                if K == 1:
                    return one
                if block is None:
                    block = torch.empty((one.shape[0], K) + tuple(one.shape[1:]), dtype=one.dtype, device=one.device)
                block[:, k] = one
        return block.reshape(block.shape[0], -1, block.shape[-1])

    if K == 1:
        return one_by_one()
    y0, t, rtol, atol, method, options = _check_inputs(func, y0s, t, rtol, atol, method, options)
    # (a grid per call is prepared as one shared grid: _prepare reads a 2-D t as one grid per TRAJECTORY)
    params, y2, t64, B, N, per_sample, t_is_f32, control = _prepare(func, y0, t[0] if grids else t, options)
    if per_sample or control != _lib.CTRL_SHARED:
        raise ValueError("odeint_calls: one shared time grid per call, batch_control='shared'")
    if grids:
        t64 = t.detach().to(device=y0.device, dtype=t64.dtype).contiguous()
    if options.get("step_size"):      # the batched launch has no sub-step loop: the K calls themselves
        return one_by_one()
    engine.check_pending_status()
    p = engine.params_cached(*params)
    try:
        sol, status, _, _ = engine.solve_forward(p, y2.detach().contiguous(), t64, method, control, rtol, atol, grids,
                                                 t_is_f32, int(options.get("max_num_steps", 0)), calls=K)
    except ValueError:
        return one_by_one()
    engine.raise_for_status(status)
    return sol


def odeint_calls(func, y0s, t, rtol=1e-7, atol=1e-9, method=None, options=None, clamp=None):
    """K forward-only `odeint(func, y0s[k], t, ...)` calls in as few launches as the device has room for:
        y0s [K, *shape] (shape = [B,1,N] or [B,N]), t [T]  ->  [K, T, *shape]  (a view of the engine's [T, K*B, N]).
    t [K, T]: one time grid per call, `odeint(func, y0s[k], t[k], ...)` -- the validation loop of train_insilico.py:77-106;
    the grids may differ in start, span and direction, and dopri5 runs on the third-generation kernels.
    Every call keeps the reference's batch semantics -- ONE adaptive step size shared by its B trajectories, chosen
    from its own error norm -- so the result equals the K separate calls (the analysis loop of
    find_gene_influences.py:64-77 issues 2 per gene).  Falls back to K launches where the batched plan does not
    exist (shapes served by the VALU engine).
    clamp (K ints, a sequence or an integer tensor; -1: none): call k holds gene clamp[k] at its initial value for the
    whole time course, d y[:, clamp[k]] / dt = 0 -- level 0 is a knockout, a high level an over-expression.  Exactly the
    solve of the model whose gene_multipliers[clamp[k]] is 0 (odenet.py:85-91).  An entry may also be a sequence of 1-4
    ints, and clamp a 2-D integer tensor [K, W <= 4] padded with -1: call k then holds every gene of its set (a
    combination knockout; widths may differ between calls, a gene named twice counts once, the empty set holds none).
    dopri5 calls that the third-generation kernels plan run in one launch (phx_odeint_clamped_sets); every other case
    (a fixed-grid method, step_size, the VALU engine, calls of more rows than those kernels plan) runs the K calls one by
    one on a cloned multiplier vector with those entries zeroed; the module is never modified.  The list is type- and
    range-checked on the host before any launch."""
    K = y0s.shape[0]
    sol = _calls_block(func, y0s, t, rtol, atol, method, options, clamp=clamp)
    return sol.reshape((sol.shape[0], K) + tuple(y0s.shape[1:])).transpose(0, 1)


def _adjoint_step(options, a_step, adjoint_method):
    """step size of the backward solve: adjoint_options["step_size"], else the forward's; none for dopri5"""
    if adjoint_method not in _FIXED_GRID_METHODS:
        return 0.0
    return options.get("step_size", 0.0) if a_step is None else a_step


def odeint_adjoint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint_rtol=None,
                   adjoint_atol=None, adjoint_method=None, adjoint_options=None, adjoint_params=None, _via_odeint=False,
                   clamp=None, _who="odeint_adjoint"):
    """adjoint.py:165-204.  Gradients flow to y0 and to the six ODENet parameters.
    clamp (None: no gene is held): per trajectory ROW b of y0 [B,1,N] / [B,N] a set of at most engine.CLAMP_MAX genes
    held at their initial values for the whole time course of that row -- perturbation time courses (knockouts at level
    0, over-expression at a high level) to train on, mixed with unperturbed rows (the empty set) in one minibatch.  B
    entries, each an int (-1: none) or a sequence of up to four ints, or an integer tensor [B] / [B, W <= 4] padded
    with -1; checked on the host before any launch.  Row b IS the solve of the model whose gene_multipliers are 0 on
    its set (odenet.py:85-91), forward and backward: d y[b, k] / dt = 0 on the set; the gradient is the continuous
    adjoint of that per-row model -- y0.grad[b, k] is dL/d(the level gene k is held at), gene_multipliers.grad[k] and
    row k of the combine layer's weight gradient receive nothing from row b; parameter gradients are summed over the
    rows.  The module is never modified.  Per-trajectory step control only (t [B, T], or options={"batch_control":
    "per_trajectory"}); with one shared controller a per-row clamp raises ValueError -- `odeint_calls`' clamp is per
    CALL, this one per ROW.  dopri5 with H <= 48 runs the per-row forms of k1_solve_fwd3 / k1_solve_adj3, one launch
    per direction; everything else (H > 48, euler / midpoint / rk4, step_size, PHX_ENGINE=v0) groups the rows by
    identical set and runs every group through the ordinary entry points on a cloned multiplier vector zeroed on the
    set, parameter gradients accumulated in the sorted order of the sets.  A list whose sets are all empty runs the
    unclamped call unchanged."""
    # adjoint_options may hold step_size and nothing else; absent, the backward solve inherits the forward's step
    # (adjoint.py:182-183: adjoint_options defaults to options)
    adjoint_options = {} if adjoint_options is None else dict(adjoint_options)
    a_step = adjoint_options.pop("step_size", None)
    if adjoint_options:
        raise NotImplementedError("phoenix_amd: adjoint_options other than step_size are not supported (got %s)"
                                  % sorted(adjoint_options))
    if a_step is not None:
        a_step = _step_size(a_step)
    if not _is_odenet(func):      # any other module: the reference's augmented system on the unfused torch stepper
        if clamp is not None:
            raise NotImplementedError("phoenix_amd: %s: clamp needs a PHOENIX ODENet" % _who)
        y0, t, rtol, atol, method, options = _check_inputs(func, y0, t, rtol, atol, method, options)
        engine._require_gpu(y0, "y0")          # like every other entry point: no CPU compute path in this package
        assert t.ndimension() == 1, "per-sample time grids need a PHOENIX ODENet"
        return generic.odeint_adjoint(func, y0, t, rtol, atol, method, options,
                                      rtol if adjoint_rtol is None else adjoint_rtol,
                                      atol if adjoint_atol is None else adjoint_atol,
                                      method if adjoint_method is None else adjoint_method, adjoint_params,
                                      options.get("step_size") if a_step is None else a_step)
    if adjoint_params is not None:
        raise NotImplementedError("phoenix_amd: adjoint_params is fixed to ODENet's six parameters")
    if adjoint_rtol is None:
        adjoint_rtol = rtol
    if adjoint_atol is None:
        adjoint_atol = atol
    y0, t, rtol, atol, method, options = _check_inputs(func, y0, t, rtol, atol, method, options)
    if adjoint_method is None:
        adjoint_method = method
    if adjoint_method not in _ENGINE_METHODS:
        raise NotImplementedError("phoenix_amd: adjoint_method '%s' not supported" % adjoint_method)
    if a_step is not None and adjoint_method not in _FIXED_GRID_METHODS:      # as options with dopri5 (misc.py:204-206)
        warnings.warn("phoenix_amd: Unexpected arguments {}".format({"step_size": a_step}))
    held = _row_clamp(_who, func, y0, t, options, clamp)
    params, y2, t64, B, N, per_sample, t_is_f32, control = _prepare(func, y0, t, options)
    # The forward status is read together with the backward solve's only when a backward pass can come: autograd must
    # be recording AND something must require grad (needs_input_grad mirrors .requires_grad even under no_grad: the
    # reference's validation code calls odeint_adjoint inside torch.no_grad(), train_insilico.py:77-106).
    # (a plain `odeint` call routed here keeps the reference's synchronous asserts: its caller may never run backward)
    # ... except with a fixed-grid method, whose backward pass (backpropagation through the steps) reads both together
    defer = (torch.is_grad_enabled() and (y0.requires_grad or any(x.requires_grad for x in params)) and
             (not _via_odeint or adjoint_method in _FIXED_GRID_METHODS))
    cfg = (method, control, rtol, atol, per_sample, t_is_f32, int(options.get("max_num_steps", 0)),
           (adjoint_method, float(adjoint_rtol), float(adjoint_atol), bool(_via_odeint)), defer,
           (options.get("step_size", 0.0), _adjoint_step(options, a_step, adjoint_method)))
    sol, _nfe = _OdeintAdjointFn.apply(y2, t64, cfg, *params, held)
    return _out_shape(sol, y0, per_sample)


def odeint_per_sample(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint=True, clamp=None):
    """The reference's per-sample python loop as ONE launch:
        for time, batch_point in zip(t, batch): odeint(odenet, batch_point, time, method)[1]
    y0 [B,1,N] (or [B,N]), t [B,T]; returns [T, *y0.shape]; independent step control per sample.
    clamp: the genes sample b holds for its whole time course, one entry per sample (`odeint_adjoint`)."""
    assert t.ndimension() == 2, "odeint_per_sample needs t of shape [B, T]"
    if adjoint:
        return odeint_adjoint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options, clamp=clamp,
                              _who="odeint_per_sample")
    return odeint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options, clamp=clamp)
