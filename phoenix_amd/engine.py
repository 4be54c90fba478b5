"""Thin torch <-> C-ABI glue: device pointers, the current HIP stream, caller-owned workspaces.

PyTorch here is plumbing (device memory, streams, autograd bookkeeping); all arithmetic of the
path happens in libphoenix_hip.so."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

_ws_cache = {}


def _require_gpu(x, name):
    if not x.is_cuda:
        raise RuntimeError("phoenix_amd: `%s` must live on the GPU (cuda/HIP device); this engine has no CPU path"
                           % name)
    if x.is_floating_point() and x.dtype != torch.float32:
        raise TypeError("phoenix_amd: `%s` must be float32 (got %s); the engine computes in float32 like the "
                        "reference's configs" % (name, x.dtype))


# The host side of a step is a few hundred microseconds of Python, which is what a small-batch step costs on a slow host
# (17 trajectories at the breast-cancer shape: 0.32 ms of kernels): the current stream and the plan switches are read
# through the cheapest route there is (torch.cuda.current_stream() builds a Stream object through four Python frames, 8 us;
# os.environ.get encodes and decodes, 0.8 us per switch, and a solve reads all of them several times).
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_raw(device_index=None):
    """handle (an int) of the current HIP stream of `device_index` (default: the current device)"""
    if _raw_stream is None or _raw_device is None:
        return torch.cuda.current_stream(device_index).cuda_stream
    return _raw_stream(_raw_device() if device_index is None else device_index)


def _stream_ptr():
    return C.c_void_p(_stream_raw())


_ws_bytes = {}
_PLAN_ENV = ("PHX_ENGINE", "PHX_ADJ", "PHX_ADJ2_NP", "PHX_V1_MAXNW", "PHX_PGRAD", "PHX_EVAL_NBC", "PHX_PGRAD_KS", "PHX_FWD", "PHX_V3_NB",
             "PHX_V3_HALF", "PHX_BATCH_MIN_ROWS", "PHX_PGRAD_WGS", "PHX_PGRAD_G4", "PHX_BATCH_CHUNK_MIN", "PHX_V3C", "PHX_V3C_NB",
             "PHX_V3C_TPW", "PHX_V3C_RES", "PHX_V3C_SLOTS", "PHX_V3C_HB", "PHX_V3C_NTG", "PHX_V3C_SPLIT")


_PLAN_ENV_B = tuple(os.fsencode(k) for k in _PLAN_ENV)
_env_data = getattr(os.environ, "_data", None)


def _plan_env():
    """the values of the plan switches (part of every plan / workspace key: the tests and tools flip them between calls)"""
    if isinstance(_env_data, dict) and os.name == "posix":
        return tuple(map(_env_data.get, _PLAN_ENV_B))     # bytes or None: only compared with itself
    return tuple(os.environ.get(k) for k in _PLAN_ENV)


# phx_solve_opts.ws_keep: what the previous solve on a cached workspace was (plan key), so that the next identical one can
# vouch for the workspace and the library skips the fill of its exchange buffers (the third-generation kernels alternate
# between two sets and clean the idle one themselves).  Any other use drops the entry: the next call fills as usual.
_ws_last = {}


def forget_params():
    """drops the cached engine layouts of parameter tensors (`params_cached`): for a caller that changed parameters behind
    PyTorch's version counters -- a replayed graph that contains the optimizer step does"""
    _params_cache.clear()


def forget_workspaces():
    """for a caller that writes into the cached workspaces itself (the tests poison them): the next solves zero-fill
    their exchange buffers again instead of vouching for what the workspace holds"""
    _ws_last.clear()


def _ws_size(key, query, *args):
    """the library's workspace-size function `query` of `args`, remembered under `key`: a size query re-plans the launch on
    the host (the keys of the solves carry the plan switches, `_plan_env`)"""
    nbytes = _ws_bytes.get(key)
    if nbytes is None:
        nbytes = _ws_bytes[key] = getattr(_lib.load(), query)(*args)
    return nbytes


def _stream_buffer(op, nbytes, device, grow=1, slack=1024, solve=False):
    """the cached uint8 buffer of `op` on the current stream of `device`, at least `nbytes` long; a new one gets
    nbytes * grow + slack.  solve: the buffer is a solve workspace, and a new one is in no vouched-for state (`_ws_last`)"""
    key = (device.index, _stream_raw(device.index), op)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _ws_cache[key] = torch.empty(int(nbytes * grow) + slack, dtype=torch.uint8, device=device)
        if solve:
            _ws_last.pop(key, None)
    return buf


def _workspace(op, N, H, B, T, device, calls=1, grids_method=None):
    # grids_method: the calls have a time grid each (phx_odeint_calls_grids_workspace_bytes depends on the method)
    key = (op, N, H, B, T, calls, grids_method) + _plan_env()
    if calls == 1:
        nbytes = _ws_size(key, "phx_workspace_bytes", op, N, H, B, T)
    elif grids_method is not None:
        nbytes = _ws_size(key, "phx_odeint_calls_grids_workspace_bytes", N, H, B, T, calls, _lib.METHODS[grids_method])
    else:
        nbytes = _ws_size(key, "phx_odeint_calls_workspace_bytes", N, H, B, T, calls)
    if calls > 1 and nbytes == 0:
        raise ValueError("a batch of %d calls x %d trajectories cannot be planned for N=%d, H=%d" %
                         (calls, B // calls, N, H))
    return _stream_buffer(op, nbytes, device, grow=1.25, solve=True), nbytes


def _analysis_workspace(op, nbytes, device):
    """the cached uint8 workspace of the analysis op `op` on the current stream of `device`, at least `nbytes` long (the
    callers that read counters from it view it as int32)"""
    return _stream_buffer(op, nbytes, device)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Params:
    """Device-side view of ODENet parameters in the engine layout (include/phoenix_hip.h)."""

    def __init__(self, Ws, bs, Wp, bp, Wa, g):
        for n, x in (("Ws", Ws), ("bs", bs), ("Wp", Wp), ("bp", bp), ("Wa", Wa), ("g", g)):
            _require_gpu(x, n)
            if x.dtype != torch.float32:
                raise TypeError("phoenix_amd: parameter %s must be float32 (got %s)" % (n, x.dtype))
        self.H, self.N = Ws.shape
        assert Wp.shape == (self.H, self.N) and Wa.shape == (self.N, 2 * self.H), "not a PHOENIX ODENet"
        self.Ws = Ws.detach().contiguous()
        self.bs = bs.detach().contiguous()
        self.Wp = Wp.detach().contiguous()
        self.bp = bp.detach().contiguous()
        self.g = g.detach().reshape(-1).contiguous()
        self.device = Ws.device
        # The engine layout of this parameter version in ONE kernel (phx_layout_params, ABI 6), straight from
        # net_alpha_combine.linear_out.weight as PyTorch stores it ([N, 2H]): the gene-contiguous transpose WaT [2H, N]
        # and the packed LDS weight images (phx_params.wimg) that the forward and the backward solve of a step share.
        wa = Wa.detach().contiguous()
        self.WaT = torch.empty((2 * self.H, self.N), dtype=torch.float32, device=self.device)
        nbytes = _lib.load().phx_weight_image_bytes(self.N, self.H)
        self.wimg = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if nbytes else None
        _check_call(_lib.load().phx_layout_params(_p(self.Ws), _p(self.Wp), _p(wa), _p(self.g), self.N, self.H,
                                                  _p(self.WaT), _p(self.wimg), _stream_ptr()))
        self.c = _lib.PhxParams(_p(self.Ws), _p(self.bs), _p(self.Wp), _p(self.bp), _p(self.WaT), _p(self.g),
                                self.N, self.H, self.wimg.data_ptr() if nbytes else None)
        # ready event, unconditionally: the contiguous / transposed copies above are written on this stream too
        self._ready_stream = torch.cuda.current_stream()
        self._ready_raw = self._ready_stream.cuda_stream
        self._ready_event = torch.cuda.Event()
        self._ready_event.record()

    def on_current_stream(self):
        """a call on another stream than the one that laid these parameters out waits for the layout (copies and
        packed images) and keeps their memory alive for that stream"""
        if _stream_raw(self.device.index) == self._ready_raw:
            return self
        cur = torch.cuda.current_stream()
        if cur != self._ready_stream:
            cur.wait_event(self._ready_event)
            for x in (self.Ws, self.bs, self.Wp, self.bp, self.WaT, self.g, self.wimg):
                if x is not None:
                    x.record_stream(cur)
        return self

    def new_grads(self):
        return Grads(self)


_params_cache = {}


def params_cached(Ws, bs, Wp, bp, Wa, g):
    """`Params` of these six tensors, rebuilt only when one of them changed (storage or in-place version): the engine
    layout needs a transposed copy of Wa (7 MB at breast scale), which a forward/backward pair, a validation loop or an
    analysis scan over fixed weights should not redo per call.  An optimizer step bumps the versions."""
    key = tuple((x.data_ptr(), x._version, tuple(x.shape)) for x in (Ws, bs, Wp, bp, Wa, g))
    dkey = (Ws.device.index, Ws.data_ptr())
    hit = _params_cache.get(dkey)
    if hit is not None and hit[0] == key:
        return hit[1]
    p = Params(Ws, bs, Wp, bp, Wa, g)
    if len(_params_cache) > 8:
        _params_cache.clear()
    _params_cache[dkey] = (key, p)
    return p


def invalidate_params():
    """forget the cached engine-layout copies of parameters.  Needed only after writing a parameter through a view that
    does not bump its version counter (`p.data.copy_(...)`, a raw pointer): optimizers, `copy_`, `add_` under
    `no_grad`, `load_state_dict` all bump it and need nothing."""
    _params_cache.clear()


class Grads:
    """One flat buffer carved into the six gradient tensors, every one in the REFERENCE's layout (dWa as [N, 2H],
    phx_grads.Wa): what the engine writes is what autograd hands the optimizer, no transposed copy in between.  It is
    NOT zero-filled: the engine call it is handed to writes every element (`phx_grads.overwrite`)."""

    def __init__(self, p):
        H, N = p.H, p.N
        sizes = (H * N, H, H * N, H, 2 * H * N, N)
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=p.device)
        parts = torch.split(self.flat, sizes)
        self.Ws, self.bs, self.Wp, self.bp = parts[0].view(H, N), parts[1], parts[2].view(H, N), parts[3]
        self.Wa, self.g = parts[4].view(N, 2 * H), parts[5]
        self.c = _lib.PhxGrads(_p(self.Ws), _p(self.bs), _p(self.Wp), _p(self.bp), None, _p(self.g), 1, _p(self.Wa))

    def as_reference_layout(self, g_shape):
        """(Ws, bs, Wp, bp, Wa[N,2H], g[1,N]) gradients in the reference's parameter layouts"""
        return self.Ws, self.bs, self.Wp, self.bp, self.Wa, self.g.reshape(g_shape)


def _check_call(rc):
    if rc != 0:
        raise RuntimeError("phoenix_amd: %s" % _lib.load().phx_status_string(rc).decode())


def _raise(status, worst):
    # A launch that ended in an error (above all PHX_ERR_SYNC_TIMEOUT, whose 5 s bail-out leaves the workspace header --
    # exchange-set parity, `started` counters -- in an undefined state) must not be vouched for: the next solve on every
    # cached workspace fills its exchange buffers again (phx_solve_opts.ws_keep = 0).
    forget_workspaces()
    bad = int((status != 0).nonzero()[0].item())
    msg = "%s (trajectory %d)" % (_lib.STATUS_TEXT.get(worst, "status %d" % worst), bad)
    if worst in (1, 2, 3, 4):
        raise AssertionError(msg)
    raise RuntimeError("phoenix_amd: " + msg)


_status_mode = "immediate"
_pending = []          # (event, pinned status copy [L, B]) of solves whose status has not been read yet
captured_status = []   # "captured" mode: the device status blocks of the solves issued since the mode was set


def set_status_mode(mode):
    """"immediate" (default): a training step reads the solver status of its two launches in one blocking round trip at
    the end of backward(), as the reference raises its asserts synchronously.  "deferred": the status block is copied to
    pinned host memory behind the backward kernel and checked at a later engine call (or `check_pending_status(True)`)
    once its event has completed -- the same AssertionError, raised up to two engine calls late, and the host no longer
    idles the GPU between steps.  "captured": nothing is read at all -- every status block stays on the device and is
    appended to `captured_status`; for steps recorded into a HIP graph (phoenix_amd.graphs.GraphedStep), whose caller
    reads them after a replay (`check_captured_status`)."""
    global _status_mode
    assert mode in ("immediate", "deferred", "captured")
    if mode != "deferred":
        check_pending_status(wait=True)
    _status_mode = mode


def status_mode():
    return _status_mode


_free_host = {}        # (shape, dtype) -> pinned buffers of checked solves, reused (no pinned allocation in steady state)


def defer_status(status):
    """queue a device status block [L, B] (or [B]) for a later check"""
    if _status_mode == "captured":
        captured_status.append(status)
        return
    key = (tuple(status.shape), status.dtype)
    pool = _free_host.setdefault(key, [])
    host = pool.pop() if pool else torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
    host.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _pending.append((ev, host))


def check_pending_status(wait=False):
    """raise for every queued solve that has finished (all of them with wait=True)"""
    if _status_mode == "captured":
        return                   # (event queries and synchronisation have no place inside a capture)
    while _pending:
        ev, host = _pending[0]
        if not wait and not ev.query():
            return
        if wait:
            ev.synchronize()
        _pending.pop(0)
        pool = _free_host.setdefault((tuple(host.shape), host.dtype), [])
        if len(pool) < 8:
            pool.append(host)
        raise_for_status(host)


def check_captured_status(blocks=None):
    """reads the status blocks a captured step left on the device (default: `captured_status`) and raises like
    `raise_for_status`; one device->host read per block, outside any capture"""
    for st in (captured_status if blocks is None else blocks):
        raise_for_status(st, _force=True)


def raise_for_status(status, _force=False):
    """Maps per-trajectory solver status onto the reference's exceptions (rk_common.py:154,175-176,
    misc.py:114-115).  One device->host read.  `status` is [B], or [L, B] for L consecutive launches (the forward
    and backward solve of a training step share one stats block): the earliest failing launch is reported.
    In "captured" status mode (a step being recorded into a graph, or one of its warm-up runs) the block is kept for
    `check_captured_status` instead."""
    if _status_mode == "captured" and status.is_cuda and not _force:
        captured_status.append(status)
        return
    if status.dim() == 1:
        status = status.unsqueeze(0)
    if not status.is_cuda and not bool(status.any()):
        return
    for launch, worst in enumerate(status.amax(dim=1).tolist()):
        if worst != 0:
            _raise(status[launch], int(worst))


def rhs_forward(p, y, prior_only=False):
    _require_gpu(y, "y")
    y2 = y.detach().reshape(-1, p.N).contiguous()
    out = torch.empty_like(y2)
    B = y2.shape[0]
    p.on_current_stream()
    ws, nb = _workspace(_lib.OP_RHS_FORWARD, p.N, p.H, B, 0, y.device)
    _check_call(_lib.load().phx_rhs_forward(C.byref(p.c), _p(y2), _p(out), B, int(prior_only), _p(ws), nb,
                                            _stream_ptr()))
    return out.reshape(y.shape)


def rhs_vjp(p, y, cot, prior_only=False, want_grads=True, want_vjp_y=True, f_out=None):
    """phx_rhs_vjp on a batch; `f_out` (optional, a contiguous float32 tensor shaped like `y`) also receives f(y) --
    the C entry point's `f_out` argument."""
    _require_gpu(y, "y")
    _require_gpu(cot, "cot")
    y2 = y.detach().reshape(-1, p.N).contiguous()
    c2 = cot.detach().reshape(-1, p.N).contiguous()
    B = y2.shape[0]
    vjp = torch.empty_like(y2) if want_vjp_y else None
    grads = p.new_grads() if want_grads else None
    p.on_current_stream()
    ws, nb = _workspace(_lib.OP_RHS_VJP, p.N, p.H, B, 0, y.device)
    if f_out is not None:
        _require_gpu(f_out, "f_out")
        if f_out.dtype != torch.float32 or not f_out.is_contiguous() or f_out.numel() != y2.numel():
            raise ValueError("f_out must be a contiguous float32 tensor with as many elements as y")
    _check_call(_lib.load().phx_rhs_vjp(C.byref(p.c), _p(y2), _p(c2), _p(vjp), C.byref(grads.c) if grads else None,
                                        _p(f_out) if f_out is not None else C.c_void_p(0), B, int(prior_only), _p(ws), nb,
                                        _stream_ptr()))
    return (vjp.reshape(y.shape) if want_vjp_y else None), grads


PRIOR_MSE_MIN_ROWS = 1024   # the fused loss head is for the large prior batches (train_insilico.py:134); smaller ones take the plain formula


def prior_mse(p, X, target, keep_hidden=False):
    """fused mean((prior_only_forward(X) - target)^2) and its cotangent; returns (loss [1], cot like X) -- with
    `keep_hidden` (loss, cot, z): z = what `prior_vjp_saved` needs of the hidden layer (since ABI 7 the four sections
    du | dv | z_u | z_p of every row, formed with THIS cotangent), or None where the library has no such path (H > 128) -- or None when the engine cannot plan the batch chain for this shape
    (caller falls back to the unfused formula)."""
    _require_gpu(X, "X")
    _require_gpu(target, "target")
    x2 = X.detach().reshape(-1, p.N).contiguous()
    t2 = target.detach().reshape(-1, p.N).contiguous()
    B = x2.shape[0]
    if B < PRIOR_MSE_MIN_ROWS or t2.shape != x2.shape:
        return None
    cot = torch.empty_like(x2)
    loss = torch.empty(1, dtype=torch.float32, device=x2.device)
    p.on_current_stream()
    ws, nb = _workspace(_lib.OP_RHS_FORWARD, p.N, p.H, B, 0, X.device)
    zbytes = _lib.load().phx_prior_z_bytes(p.N, p.H, B) if keep_hidden else 0
    if zbytes:
        z = torch.empty(zbytes // 4, dtype=torch.float32, device=x2.device)
        rc = _lib.load().phx_prior_mse_save(C.byref(p.c), _p(x2), _p(t2), B, _p(cot), _p(loss), _p(z), _p(ws), nb,
                                            _stream_ptr())
    else:
        z = None
        rc = _lib.load().phx_prior_mse(C.byref(p.c), _p(x2), _p(t2), B, _p(cot), _p(loss), _p(ws), nb, _stream_ptr())
    if rc == 4:
        return None
    _check_call(rc)
    return (loss, cot, z) if keep_hidden else (loss, cot)


def prior_vjp_saved(p, X, cot, z):
    """parameter gradients of sum(cot * prior_only_forward(X)) from the hidden sections `z` that `prior_mse(...,
    keep_hidden=True)` kept (phx_prior_vjp_saved): what rhs_vjp(prior_only=True, want_vjp_y=False) returns, with the
    gradient contraction alone.  `cot` must be the cotangent that same call returned (z holds du, dv formed with it)."""
    _require_gpu(X, "X")
    _require_gpu(cot, "cot")
    x2 = X.detach().reshape(-1, p.N).contiguous()
    c2 = cot.detach().reshape(-1, p.N).contiguous()
    B = x2.shape[0]
    # `z` must be the buffer prior_mse(keep_hidden=True) filled for THIS batch size: the kernels index it by tile
    zbytes = _lib.load().phx_prior_z_bytes(p.N, p.H, B)
    if (z is None or not z.is_cuda or z.dtype != torch.float32 or not z.is_contiguous() or zbytes == 0 or
            z.numel() * 4 != zbytes):
        raise ValueError("prior_vjp_saved: `z` is not the hidden-row buffer of prior_mse(keep_hidden=True) for a batch "
                         "of %d rows (N=%d, H=%d)" % (B, p.N, p.H))
    grads = p.new_grads()
    p.on_current_stream()
    ws, nb = _workspace(_lib.OP_RHS_VJP, p.N, p.H, B, 0, X.device)
    _check_call(_lib.load().phx_prior_vjp_saved(C.byref(p.c), _p(x2), _p(c2), _p(z), C.byref(grads.c), B, _p(ws), nb,
                                                _stream_ptr()))
    return grads


def _opts(method, control, rtol, atol, t_per_sample, t_is_f32, max_num_steps, calls=1, ws_keep=0):
    return _lib.PhxSolveOpts(_lib.METHODS[method], control, float(rtol), float(atol), int(t_per_sample),
                             int(t_is_f32), int(max_num_steps), int(calls), int(ws_keep))


def _solve_call(op, pkey, device, call):
    """runs `call(ws_keep)` (the C entry point) and keeps the workspace bookkeeping of ws_keep"""
    wkey = (device.index, _stream_raw(device.index), op)
    keep = 1 if _ws_last.get(wkey) == pkey else 0
    _ws_last.pop(wkey, None)              # whatever happens below, the workspace is no longer in its previous state
    _check_call(call(keep))
    _ws_last[wkey] = pkey


STEPPED_MAX_STEPS = 1000000   # default budget of grid steps (per call forward, per interval backward) under a step size


def require_stepped_kernels(p, B, T, method, forward=True, backward=True):
    """raises unless kernels with the sub-step loop plan this shape, in the directions asked for: before any launch, so
    that a training step is not refused between its forward and its backward solve"""
    lib, m = _lib.load(), _lib.METHODS[method] | 0x100
    if forward and lib.phx_debug_forward_kernel_m(p.N, p.H, B, T, _lib.CTRL_PER_TRAJECTORY, m) == 0:
        raise RuntimeError("phoenix_amd: bad argument: no forward kernel with the sub-step loop of options['step_size'] "
                           "serves N=%d, H=%d under the current plan switches" % (p.N, p.H))
    if backward and lib.phx_debug_adjoint_kernel_m(p.N, p.H, B, T, _lib.CTRL_PER_TRAJECTORY, m) == 0:
        raise RuntimeError("phoenix_amd: bad argument: no backward kernel with the sub-step loop of options['step_size'] "
                           "serves N=%d, H=%d under the current plan switches" % (p.N, p.H))


# Backpropagation through the steps of options["step_size"] (solve_backprop) keeps the start state of every grid step:
# K * B * N * 4 bytes for K steps.  The cap is what one backward pass may ask for: 1 GiB, i.e. ~3000 steps of 256
# trajectories at the in-silico scale (N = 350) and 90 steps of 256 trajectories at breast-cancer scale (N = 11165) -- far
# above what a fixed grid is chosen for (a handful of steps per interval), well below the device's memory, so that a
# mistyped step size is refused at the call instead of allocating tens of gigabytes.
BACKPROP_MAX_CHECKPOINT_BYTES = 1 << 30


def backprop_grid_steps(t64, step_size):
    """largest number of grid steps any trajectory of t64 ([T] or [B, T], in the dtype the engine reads) takes under
    `step_size` -- the count phx_odeint_stepped's grid has (solvers.py:59-71: ceil((t_end - t_0) / h + 1) points, formed
    in the dtype of t); one read of the device when t lives there"""
    if t64.shape[-1] < 2:
        return 1
    q = ((t64[..., -1] - t64[..., 0]).abs() / step_size + 1).ceil().max().item()
    if not q == q or q > 2147483000.0:      # non-finite t: the kernel reports it
        return 2147483000 if q == q else 1
    return max(int(q) - 1, 1)


def require_backprop(N, H, B, T, method, t64=None, step_size=0.0):
    """raises unless the backward pass of `odeint(method=<fixed grid>)` can serve this call, before anything is launched:
    the kernel must plan the shape (H <= 128, not PHX_ENGINE=v0) and the checkpoints of a step size must fit
    BACKPROP_MAX_CHECKPOINT_BYTES.  Returns the number of grid steps to size the workspace for (0: no step size)."""
    if _lib.load().phx_debug_backprop_kernel_m(N, H, B, T, _lib.METHODS[method]) == 0:
        raise RuntimeError("phoenix_amd: bad argument: backpropagation through odeint(method='%s') serves hidden layers "
                           "up to H = 128 on the MFMA engine; N=%d, H=%d under the current plan switches is not served "
                           "(use odeint_adjoint, the continuous adjoint)" % (method, N, H))
    step = _step_of(method, step_size)
    if not step:
        return 0
    K = backprop_grid_steps(t64, step)
    if K * B * N * 4 > BACKPROP_MAX_CHECKPOINT_BYTES:
        raise RuntimeError("phoenix_amd: backpropagation through %d grid steps of step_size=%g needs %d bytes of "
                           "checkpoints (steps x %d trajectories x %d genes x 4), over the cap "
                           "engine.BACKPROP_MAX_CHECKPOINT_BYTES = %d; use a larger step, or odeint_adjoint"
                           % (K, step, K * B * N * 4, B, N, BACKPROP_MAX_CHECKPOINT_BYTES))
    return K


def _step_of(method, step_size):
    """the step size the stepped entry points get: 0.0 (= the plain entry point's behaviour) unless a fixed-grid method"""
    return float(step_size) if step_size and method != "dopri5" else 0.0


def solve_forward(p, y0, t64, method, control, rtol, atol, t_per_sample, t_is_f32, max_num_steps=0, stats=None,
                  calls=1, step_size=0.0):
    """y0 [B,N] f32, t64 [T] or [B,T] f64 (device) -> sol [T,B,N], status[B], nfe[B], nsteps[B].
    The engine writes NaN into the outputs a failed trajectory never reached (a backward solve launched before the
    status is read then stops at once).  calls > 1 (shared control): the rows are `calls` independent odeint calls
    of B/calls rows each, every call with its own step controller (include/phoenix_hip.h, phx_solve_opts.calls);
    with t_per_sample, t64 is [calls, T], one grid per call.  ValueError where no batched plan exists.
    step_size > 0 (fixed-grid methods): options["step_size"], phx_odeint_stepped."""
    B, N = y0.shape
    step = _step_of(method, step_size)
    if step and calls > 1:
        raise ValueError("calls > 1 has no sub-step loop")
    if step and not max_num_steps:
        max_num_steps = STEPPED_MAX_STEPS
    if calls > 1 and (control != _lib.CTRL_SHARED or B % calls):
        raise ValueError("calls > 1 needs shared step control and B divisible by calls")
    T = t64.shape[-1]
    sol = torch.empty((T, B, N), dtype=torch.float32, device=y0.device)
    if stats is None:      # not zero-filled: every solve kernel writes status / nfe / nsteps of every trajectory
        stats = torch.empty((3, B), dtype=torch.int32, device=y0.device)
    p.on_current_stream()
    if t_per_sample and control == _lib.CTRL_SHARED and (calls <= 1 or t64.shape[0] != calls):
        raise ValueError("a shared step controller has one time grid; calls > 1 take t of shape [calls, T]")
    ws, nb = _workspace(_lib.OP_ODEINT, p.N, p.H, B, T, y0.device, calls,
                        method if calls > 1 and t_per_sample else None)
    pkey = (p.N, p.H, B, T, method, control, int(t_per_sample), calls, step) + _plan_env()

    def call(keep):
        o = _opts(method, control, rtol, atol, t_per_sample, t_is_f32, max_num_steps, calls, keep)
        if step:
            return _lib.load().phx_odeint_stepped(C.byref(p.c), _p(y0), _p(t64), B, T, C.byref(o), _p(sol), _p(stats[0]),
                                                  _p(stats[1]), _p(stats[2]), _p(ws), nb, _stream_ptr(), step)
        return _lib.load().phx_odeint(C.byref(p.c), _p(y0), _p(t64), B, T, C.byref(o), _p(sol), _p(stats[0]),
                                      _p(stats[1]), _p(stats[2]), _p(ws), nb, _stream_ptr())

    _solve_call(_lib.OP_ODEINT, pkey, y0.device, call)
    return sol, stats[0], stats[1], stats[2]


OP_CLAMPED = 11      # workspace-size key of solve_forward_clamped (phx_odeint_clamped_workspace_bytes sizes it)
CLAMP_MAX = 4        # PHX_CLAMP_MAX: the genes one call can hold


def clamped_plan_exists(N, H, B, T, calls):
    """whether phx_odeint_clamped serves `calls` dopri5 calls of B // calls rows (k1_solve_fwd3 / k1_solve_fwd3c plan
    them); the size is remembered per shape and plan-switch setting"""
    return _ws_size((OP_CLAMPED, N, H, B, T, calls) + _plan_env(), "phx_odeint_clamped_workspace_bytes", N, H, B, T, calls)


def solve_forward_clamped(p, y0, t64, clamp, rtol, atol, t_is_f32, max_num_steps=0, stats=None):
    """`solve_forward` for dopri5 under shared control with calls = len(clamp) and one grid per call (t64 [calls, T]),
    where call k holds gene clamp[k] at its initial value, or -- clamp [calls, width <= CLAMP_MAX] -- every gene of row k
    (phx_odeint_clamped_sets; an int32 device tensor, -1: none / padding).
    ValueError where no third-generation kernel plans the calls -- solve them one by one on parameters whose g is
    zeroed on the set."""
    B, N = y0.shape
    if clamp.dim() not in (1, 2) or (clamp.dim() == 2 and not 1 <= clamp.shape[1] <= CLAMP_MAX):
        raise ValueError("solve_forward_clamped: clamp must be [calls] or [calls, 1 .. %d], got %s"
                         % (CLAMP_MAX, tuple(clamp.shape)))
    calls = clamp.shape[0]
    width = clamp.shape[1] if clamp.dim() == 2 else 1
    if clamp.dtype != torch.int32 or clamp.device != y0.device or not clamp.is_contiguous():
        raise ValueError("solve_forward_clamped: clamp must be a contiguous int32 tensor on y0's device")
    if calls < 1 or B % calls or t64.dim() != 2 or t64.shape[0] != calls:
        raise ValueError("solve_forward_clamped: B divisible by the calls, t of shape [calls, T]")
    T = t64.shape[-1]
    nb = clamped_plan_exists(p.N, p.H, B, T, calls)
    if nb == 0:
        raise ValueError("a batch of %d clamped calls x %d trajectories cannot be planned for N=%d, H=%d" %
                         (calls, B // calls, N, p.H))
    sol = torch.empty((T, B, N), dtype=torch.float32, device=y0.device)
    if stats is None:
        stats = torch.empty((3, B), dtype=torch.int32, device=y0.device)
    p.on_current_stream()
    # the solve workspace of the stream, shared with solve_forward (one launch at a time uses it)
    ws = _stream_buffer(_lib.OP_ODEINT, nb, y0.device, grow=1.25, solve=True)
    pkey = ("clamped", p.N, p.H, B, T, calls) + _plan_env()

    def call(keep):
        o = _opts("dopri5", _lib.CTRL_SHARED, rtol, atol, 1, t_is_f32, max_num_steps, calls, keep)
        return _lib.load().phx_odeint_clamped_sets(C.byref(p.c), _p(y0), _p(t64), B, T, C.byref(o), _p(clamp), width,
                                                   _p(sol), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(ws), nb,
                                                   _stream_ptr())

    _solve_call(_lib.OP_ODEINT, pkey, y0.device, call)
    return sol, stats[0], stats[1], stats[2]


def clamped_rows_plan_exists(op, N, H, B, T, method="dopri5"):
    """whether the per-row clamp kernels serve a batch of B rows in direction `op` (_lib.OP_ODEINT / OP_ADJOINT): dopri5
    with H <= 48 where k1_solve_fwd3 / k1_solve_adj3 plan the shape (phx_odeint_clamped_rows_workspace_bytes, 0: not
    served; any other method: not served); the size is remembered per shape and plan-switch setting"""
    if method != "dopri5":
        return 0
    return _ws_size(("clamped_rows", op, N, H, B, T) + _plan_env(), "phx_odeint_clamped_rows_workspace_bytes", op, N, H, B, T)


def _check_row_clamp(name, clamp, B, device):
    if (clamp.dim() != 2 or clamp.shape[0] != B or not 1 <= clamp.shape[1] <= CLAMP_MAX or clamp.dtype != torch.int32 or
            clamp.device != device or not clamp.is_contiguous()):
        raise ValueError("%s: clamp must be a contiguous int32 tensor [B = %d, 1 .. %d] on the solve's device"
                         % (name, B, CLAMP_MAX))


def solve_forward_clamped_rows(p, y0, t64, clamp, rtol, atol, t_per_sample, t_is_f32, max_num_steps=0, stats=None):
    """`solve_forward` for dopri5 under per-trajectory control where row b holds the genes clamp[b] (int32 device tensor
    [B, width <= CLAMP_MAX], -1: padding; an all -1 row is an unperturbed sample) at their initial values
    (phx_odeint_clamped_rows).  ValueError where `clamped_rows_plan_exists` is 0."""
    B, N = y0.shape
    _check_row_clamp("solve_forward_clamped_rows", clamp, B, y0.device)
    T = t64.shape[-1]
    nb = clamped_rows_plan_exists(_lib.OP_ODEINT, p.N, p.H, B, T)
    if nb == 0:
        raise ValueError("no kernel holds genes per row for N=%d, H=%d, B=%d" % (N, p.H, B))
    sol = torch.empty((T, B, N), dtype=torch.float32, device=y0.device)
    if stats is None:
        stats = torch.empty((3, B), dtype=torch.int32, device=y0.device)
    p.on_current_stream()
    ws = _stream_buffer(_lib.OP_ODEINT, nb, y0.device, grow=1.25, solve=True)      # the stream's forward solve workspace
    pkey = ("clamped_rows", p.N, p.H, B, T, int(t_per_sample)) + _plan_env()

    def call(keep):
        o = _opts("dopri5", _lib.CTRL_PER_TRAJECTORY, rtol, atol, t_per_sample, t_is_f32, max_num_steps, 1, keep)
        return _lib.load().phx_odeint_clamped_rows(C.byref(p.c), _p(y0), _p(t64), B, T, C.byref(o), _p(clamp),
                                                   clamp.shape[1], _p(sol), _p(stats[0]), _p(stats[1]), _p(stats[2]),
                                                   _p(ws), nb, _stream_ptr())

    _solve_call(_lib.OP_ODEINT, pkey, y0.device, call)
    return sol, stats[0], stats[1], stats[2]


def solve_adjoint_clamped_rows(p, t64, y_saved, grad_y, clamp, rtol, atol, t_per_sample, t_is_f32, want_grads=True,
                               max_num_steps=0, stats=None):
    """`solve_adjoint` for dopri5 under per-trajectory control of the per-row model of `solve_forward_clamped_rows`:
    the continuous adjoint of row b is that of the model with g zeroed on clamp[b]
    (phx_odeint_adjoint_backward_clamped_rows).  ValueError where `clamped_rows_plan_exists` is 0."""
    T, B, N = y_saved.shape
    _check_row_clamp("solve_adjoint_clamped_rows", clamp, B, y_saved.device)
    nb = clamped_rows_plan_exists(_lib.OP_ADJOINT, p.N, p.H, B, T)
    if nb == 0:
        raise ValueError("no backward kernel holds genes per row for N=%d, H=%d, B=%d" % (N, p.H, B))
    adj = torch.empty((B, N), dtype=torch.float32, device=y_saved.device)
    if stats is None:
        stats = torch.empty((3, B), dtype=torch.int32, device=y_saved.device)
    grads = p.new_grads() if want_grads else None
    p.on_current_stream()
    ws = _stream_buffer(_lib.OP_ADJOINT, nb, y_saved.device, grow=1.25, solve=True)
    pkey = ("clamped_rows", p.N, p.H, B, T, int(t_per_sample), bool(want_grads)) + _plan_env()

    def call(keep):
        o = _opts("dopri5", _lib.CTRL_PER_TRAJECTORY, rtol, atol, t_per_sample, t_is_f32, max_num_steps, 1, keep)
        return _lib.load().phx_odeint_adjoint_backward_clamped_rows(
            C.byref(p.c), _p(t64), B, T, C.byref(o), _p(clamp), clamp.shape[1], _p(y_saved), _p(grad_y), _p(adj),
            C.byref(grads.c) if grads else None, _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(ws), nb, _stream_ptr())

    _solve_call(_lib.OP_ADJOINT, pkey, y_saved.device, call)
    return adj, grads, stats[0], stats[1], stats[2]


def solve_adjoint(p, t64, y_saved, grad_y, method, control, rtol, atol, t_per_sample, t_is_f32, want_grads=True,
                  max_num_steps=0, stats=None, step_size=0.0, grads=None):
    """y_saved, grad_y [T,B,N] -> adj_y0 [B,N], Grads, status, nfe, nsteps.  `stats`: an int32 [3,B] to use (rows contiguous).
    step_size > 0 (fixed-grid methods): the backward solve's own step, phx_odeint_adjoint_backward_stepped.
    grads: a Grads to write into under its own overwrite flag (`grads.c.overwrite` = 0 adds) instead of a new one."""
    T, B, N = y_saved.shape
    step = _step_of(method, step_size)
    if step and not max_num_steps:
        max_num_steps = STEPPED_MAX_STEPS
    adj = torch.empty((B, N), dtype=torch.float32, device=y_saved.device)
    if stats is None:
        stats = torch.empty((3, B), dtype=torch.int32, device=y_saved.device)
    if grads is None:
        grads = p.new_grads() if want_grads else None
    p.on_current_stream()
    ws, nb = _workspace(_lib.OP_ADJOINT, p.N, p.H, B, T, y_saved.device)
    pkey = (p.N, p.H, B, T, method, control, int(t_per_sample), bool(want_grads), step) + _plan_env()

    def call(keep):
        o = _opts(method, control, rtol, atol, t_per_sample, t_is_f32, max_num_steps, 1, keep)
        args = (C.byref(p.c), _p(t64), B, T, C.byref(o), _p(y_saved), _p(grad_y), _p(adj),
                C.byref(grads.c) if grads else None, _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(ws), nb, _stream_ptr())
        if step:
            return _lib.load().phx_odeint_adjoint_backward_stepped(*args, step)
        return _lib.load().phx_odeint_adjoint_backward(*args)

    _solve_call(_lib.OP_ADJOINT, pkey, y_saved.device, call)
    return adj, grads, stats[0], stats[1], stats[2]


OP_BACKPROP = 4      # workspace-cache key of solve_backprop (phx_odeint_backprop_workspace_bytes sizes it, not phx_op)


def _workspace_backprop(N, H, B, T, K, device):
    nbytes = _ws_size((OP_BACKPROP, N, H, B, T, K) + _plan_env(), "phx_odeint_backprop_workspace_bytes", N, H, B, T, K)
    return _stream_buffer(OP_BACKPROP, nbytes, device, solve=True), nbytes


def solve_backprop(p, t64, y_saved, grad_y, method, control, t_per_sample, t_is_f32, want_grads=True, max_num_steps=0,
                   stats=None, step_size=0.0, grid_steps=0, grads=None):
    """backpropagation through the fixed-grid steps of the forward solve (phx_odeint_backprop_backward):
    y_saved, grad_y [T,B,N] -> adj_y0 [B,N], Grads, status, nfe, nsteps, like solve_adjoint.  `grid_steps`: what
    require_backprop returned for this call (the checkpoints of a step size).  grads: as in solve_adjoint."""
    T, B, N = y_saved.shape
    step = _step_of(method, step_size)
    if step and not max_num_steps:
        max_num_steps = STEPPED_MAX_STEPS
    adj = torch.empty((B, N), dtype=torch.float32, device=y_saved.device)
    if stats is None:
        stats = torch.empty((3, B), dtype=torch.int32, device=y_saved.device)
    if grads is None:
        grads = p.new_grads() if want_grads else None
    p.on_current_stream()
    K = int(grid_steps) if step else 0
    ws, nb = _workspace_backprop(p.N, p.H, B, T, K, y_saved.device)
    pkey = (p.N, p.H, B, T, method, control, int(t_per_sample), bool(want_grads), step, K) + _plan_env()

    def call(keep):
        o = _opts(method, control, 0.0, 0.0, t_per_sample, t_is_f32, max_num_steps, 1, keep)
        return _lib.load().phx_odeint_backprop_backward(
            C.byref(p.c), _p(t64), B, T, C.byref(o), _p(y_saved), _p(grad_y), _p(adj), C.byref(grads.c) if grads else None,
            _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(ws), nb, _stream_ptr(), step, K)

    _solve_call(OP_BACKPROP, pkey, y_saved.device, call)
    return adj, grads, stats[0], stats[1], stats[2]


OP_INFLUENCE = 5     # workspace-cache key of influence_scores (phx_influence_workspace_bytes sizes it)


def _score_block(name, what, x, T, calls, B, N, device, layout):
    """ValueError unless x is a contiguous float32 [T, calls*B, N] block on `device` (`layout`: how the message spells it)"""
    if (x.dim() != 3 or not x.is_contiguous() or x.dtype != torch.float32 or x.device != device or
            tuple(x.shape) != (T, calls * B, N)):
        raise ValueError("%s: %s must be a contiguous float32 %s block on base's device, got %s"
                         % (name, what, layout, tuple(x.shape)))


def _score_base(name, base):
    """(T, B, N) of the unperturbed solve's block, checked"""
    if base.dim() != 3 or not base.is_contiguous() or base.dtype != torch.float32:
        raise ValueError("%s: base must be a contiguous float32 [T, B, N] block, got %s" % (name, tuple(base.shape),))
    return tuple(base.shape)


def _score_outputs(name, outs, device, f32="float32 "):
    """the outputs of a scoring pass, `outs` = [(name, tensor or None, shape, wanted)]: a wanted one that is missing is
    allocated, a given one must be a contiguous float32 device tensor of the shape's size; -> the tensors (or None)"""
    res = []
    for what, x, shape, wanted in outs:
        numel = int(np.prod(shape))
        if x is None and wanted:
            x = torch.empty(shape, dtype=torch.float32, device=device)
        if x is not None:
            _require_gpu(x, what)
            if not x.is_contiguous() or x.numel() != numel or x.device != device or (f32 and x.dtype != torch.float32):
                raise ValueError("%s: `%s` must be a contiguous %stensor of %d elements on sol's device"
                                 % (name, what, f32, numel))
        res.append(x)
    return res


def influence_scores(sol, pairs, B, genes, want_targets=False, scores=None, targets=None):
    """phx_influence_scores on the engine's output block sol [T, 2*pairs*B, N] (call 2j unperturbed, 2j+1 perturbed,
    `genes[j]` the perturbed gene of pair j) -> (scores [pairs], targets [pairs, N] or None), both on the device.
    `scores` / `targets`: contiguous float32 device tensors to write into instead of fresh ones (a row range of a
    scan's result); passing `targets` implies want_targets."""
    _require_gpu(sol, "sol")
    if sol.dim() != 3 or not sol.is_contiguous() or sol.shape[1] != 2 * pairs * B:
        raise ValueError("influence_scores: sol must be a contiguous [T, 2*pairs*B, N] block, got %s for pairs=%d, B=%d"
                         % (tuple(sol.shape), pairs, B))
    T, _, N = sol.shape
    genes = [int(g) for g in genes]
    if len(genes) != pairs:
        raise ValueError("influence_scores: %d genes for %d pairs" % (len(genes), pairs))
    # (an integer output passes here as it always has: _require_gpu checks the floating-point dtypes only)
    scores, targets = _score_outputs("influence_scores", [("scores", scores, (pairs,), True),
                                                          ("targets", targets, (pairs, N), want_targets)], sol.device, f32="")
    nbytes = _ws_size((OP_INFLUENCE, T, pairs, B, N), "phx_influence_workspace_bytes", T, pairs, B, N)
    ws = _analysis_workspace(OP_INFLUENCE, nbytes, sol.device)
    _check_call(_lib.load().phx_influence_scores(_p(sol), T, pairs, B, N, (C.c_int * pairs)(*genes), _p(scores), _p(targets),
                                                 _p(ws), nbytes, _stream_ptr()))
    return scores, targets


OP_KNOCKOUT = 12     # workspace-cache key of knockout_effects (phx_knockout_effects_workspace_bytes sizes it)


def knockout_effects(base, sol, genes, want_matrices=False, scores=None, shift=None, magnitude=None):
    """phx_knockout_effects: base [T, B, N] (the unperturbed solve), sol [T, K*B, N] (K clamped calls of B rows, `genes[k]`
    the clamped gene of call k) -> (scores [K], shift [K, N] or None, magnitude [K, N] or None), all on the device.
    `scores` / `shift` / `magnitude`: contiguous float32 device tensors to write into instead of fresh ones (a row range
    of a screen's result); passing one of the matrices implies that matrix."""
    _require_gpu(base, "base")
    _require_gpu(sol, "sol")
    genes = [int(g) for g in genes]
    K = len(genes)
    T, B, N = _score_base("knockout_effects", base)
    _score_block("knockout_effects", "sol", sol, T, K, B, N, base.device, "[T, K*B, N] = %s" % ((T, K * B, N),))
    outs = [("scores", scores, (K,), True), ("shift", shift, (K, N), want_matrices),
            ("magnitude", magnitude, (K, N), want_matrices)]
    scores, shift, magnitude = _score_outputs("knockout_effects", outs, sol.device)
    nbytes = _ws_size((OP_KNOCKOUT, T, K, B, N), "phx_knockout_effects_workspace_bytes", T, K, B, N)
    ws = _analysis_workspace(OP_KNOCKOUT, nbytes, sol.device)
    _check_call(_lib.load().phx_knockout_effects(_p(base), _p(sol), T, K, B, N, (C.c_int * K)(*genes), _p(scores), _p(shift),
                                                 _p(magnitude), _p(ws), nbytes, _stream_ptr()))
    return scores, shift, magnitude


OP_EPISTASIS = 13    # workspace-cache key of knockout_epistasis (phx_knockout_epistasis_workspace_bytes sizes it)


def knockout_epistasis(base, singles, sol, ia, ib, genes, want_matrices=False, out=None):
    """phx_knockout_epistasis: base [T, B, N] (the unperturbed solve), singles [T, G*B, N] (G single-gene calls, `genes[g]`
    the held gene of single g), sol [T, K*B, N] (K pair calls, pair k holding the genes of singles ia[k] and ib[k]) ->
    (scores [K], interaction_scores [K], shift, magnitude, interaction, interaction_magnitude), the four matrices [K, N] or
    None, all on the device.  `out`: six contiguous float32 device tensors (or None) to write into instead of fresh ones
    (a row range of a screen's result), in that order; passing a matrix implies that matrix."""
    _require_gpu(base, "base")
    _require_gpu(singles, "singles")
    _require_gpu(sol, "sol")
    ia, ib, genes = [int(i) for i in ia], [int(i) for i in ib], [int(g) for g in genes]
    K, G = len(ia), len(genes)
    if len(ib) != K:
        raise ValueError("knockout_epistasis: %d first and %d second indices" % (K, len(ib)))
    T, B, N = _score_base("knockout_epistasis", base)
    for name, x, calls in (("singles", singles, G), ("sol", sol, K)):
        _score_block("knockout_epistasis", name, x, T, calls, B, N, base.device, (T, calls * B, N))
    out = list(out) if out is not None else [None] * 6
    if len(out) != 6:
        raise ValueError("knockout_epistasis: `out` names six tensors (or None)")
    names = ("scores", "interaction_scores", "shift", "magnitude", "interaction", "interaction_magnitude")
    out = _score_outputs("knockout_epistasis", [(names[i], out[i], (K,) if i < 2 else (K, N), i < 2 or want_matrices)
                                                for i in range(6)], sol.device)
    nbytes = _ws_size((OP_EPISTASIS, T, K, G, B, N), "phx_knockout_epistasis_workspace_bytes", T, K, G, B, N)
    ws = _analysis_workspace(OP_EPISTASIS, nbytes, sol.device)
    _check_call(_lib.load().phx_knockout_epistasis(_p(base), _p(singles), _p(sol), T, K, G, B, N, (C.c_int * K)(*ia),
                                                   (C.c_int * K)(*ib), (C.c_int * G)(*genes), _p(out[0]), _p(out[1]),
                                                   _p(out[2]), _p(out[3]), _p(out[4]), _p(out[5]), _p(ws), nbytes,
                                                   _stream_ptr()))
    return tuple(out)


OP_EFFECTS = 6       # workspace-cache key of effects_matrix (phx_effects_workspace_bytes sizes it)


def int_list(name, xs, what="genes"):
    """`xs` (a sequence or an array) as a list of ints; TypeError on a bool or anything that is no integer"""
    xs = list(xs.tolist() if hasattr(xs, "tolist") else xs)
    for g in xs:
        if isinstance(g, bool) or not hasattr(g, "__index__"):
            raise TypeError("%s: %s must be integers, got %r" % (name, what, g))
    return [int(g) for g in xs]


def check_genes(name, genes, N, lowest=0):
    """ValueError unless every gene is one of lowest .. N - 1"""
    for g in genes:
        if g < lowest or g >= N:
            raise ValueError("%s: gene %d is not one of %d .. %d" % (name, g, lowest, N - 1))


def gene_values(name, value, n):
    """`value`, a scalar or one level per gene, as a list of n floats"""
    values = value.tolist() if hasattr(value, "tolist") else value
    if isinstance(values, (list, tuple)):
        if len(values) != n:
            raise ValueError("%s: %d values for %d genes" % (name, len(values), n))
        return [float(v) for v in values]
    return [float(values)] * n


def check_rows(rows, N):
    """(row0, row1) of a `rows` argument: None (all N rows) or a pair with 0 <= row0 < row1 <= N"""
    if rows is None:
        return 0, N
    try:
        row0, row1 = rows
        row0, row1 = int(row0), int(row1)
    except (TypeError, ValueError):
        raise ValueError("rows must be None or (row0, row1), got %r" % (rows,))
    if not 0 <= row0 < row1 <= N:
        raise ValueError("rows must satisfy 0 <= row0 < row1 <= %d, got %r" % (N, rows))
    return row0, row1


def _require_f32(x, name):
    """a device buffer the kernel reads or writes as float: any other dtype (an integer one passes _require_gpu) would be
    read or written past its end"""
    _require_gpu(x, name)
    if x.dtype != torch.float32:
        raise TypeError("phoenix_amd: `%s` must be float32 (got %s)" % (name, x.dtype))


def _effects_states(name, params, mode, y, ph, pairs):
    """(y, ph, B) of a call on the effects tile engine, checked: the mode, with `pairs` the shapes whose gene pairs fit the
    32-bit keys of the selecting kernels, and for the Jacobian modes the states y [B, N] and ph [B, H]"""
    if mode not in _lib.EFFECTS_MODES:
        raise ValueError("%s: mode must be one of %s, got %r" % (name, sorted(_lib.EFFECTS_MODES), mode))
    N, H = params.N, params.H
    if pairs and (H > 256 or N > 65535):
        raise ValueError("%s: H <= 256 and N <= 65535 are served, got N=%d, H=%d" % (name, N, H))
    if mode == "effects":
        return None, None, 1
    if y is None or ph is None:
        raise ValueError("%s: mode %r needs the states `y` [B, N] and `ph` [B, H]" % (name, mode))
    _require_f32(y, "y")
    _require_f32(ph, "ph")
    B = y.shape[0] if y.dim() == 2 else 0
    if B < 1 or y.shape[1] != N or tuple(ph.shape) != (B, H) or not y.is_contiguous() or not ph.is_contiguous() or \
            y.device != params.device or ph.device != params.device:
        raise ValueError("%s: y must be a contiguous [B, %d] and ph a contiguous [B, %d] tensor on the "
                         "parameters' device, got %s and %s" % (name, N, H, tuple(y.shape), tuple(ph.shape)))
    return y, ph, B


def _edges_flags(orient, diagonal):
    return (_lib.EDGES_ORIENT if orient else 0) | (_lib.EDGES_DIAGONAL if diagonal else 0)


def _check_threshold(name, threshold):
    """ValueError unless `threshold` is None or a positive, finite number"""
    if threshold is not None and not (isinstance(threshold, (int, float, np.integer, np.floating)) and
                                      not isinstance(threshold, bool) and threshold > 0 and np.isfinite(threshold)):
        raise ValueError("%s: threshold must be positive and finite, got %r" % (name, threshold))


def effects_matrix(params, mode, y=None, ph=None, rows=None, out=None):
    """phx_effects_matrix on laid-out parameters (`Params`): rows [row0, row1) of the regulator -> target matrix of `mode`
    ("effects": extract_model_matrix_PHOENIX.py:46-58; "mean" / "mean_abs": the RHS Jacobian averaged over the states
    y [B, N] as it is / in absolute value, with ph [B, H] the product-branch hidden vector of those states) -> float32
    [row1 - row0, N] on the device.  `rows`: None (all N) or (row0, row1).  `out`: a contiguous float32 device tensor of
    that shape to write into instead of a fresh one."""
    N, H = params.N, params.H
    row0, row1 = check_rows(rows, N)
    y, ph, B = _effects_states("effects_matrix", params, mode, y, ph, pairs=False)
    if out is None:
        out = torch.empty((row1 - row0, N), dtype=torch.float32, device=params.device)
    else:
        _require_f32(out, "out")
        if tuple(out.shape) != (row1 - row0, N) or not out.is_contiguous() or out.device != params.device:
            raise ValueError("effects_matrix: `out` must be a contiguous [%d, %d] tensor on the parameters' device"
                             % (row1 - row0, N))
    nbytes = _ws_size((OP_EFFECTS, N, H, B, mode), "phx_effects_workspace_bytes", N, H, B, _lib.EFFECTS_MODES[mode])
    ws = _analysis_workspace(OP_EFFECTS, nbytes, params.device) if nbytes else None
    p = params.on_current_stream()
    _check_call(_lib.load().phx_effects_matrix(C.byref(p.c), _lib.EFFECTS_MODES[mode], _p(y), _p(ph), B, row0, row1, _p(out),
                                               _p(ws), nbytes, _stream_ptr()))
    return out


OP_EDGES = 7         # workspace-cache key of effects_edges (phx_effects_edges_workspace_bytes sizes it)
EDGES_REFINE_MIN = 1 << 20    # a cut bin with more entries than max(4 K, this) is refined on the next 12 bits


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def _edges_tau(threshold):
    """the smallest float32 that is >= threshold (|M| >= threshold for a float32 M means |M| >= that), or None when
    there is none"""
    t = np.float32(threshold)
    if float(t) < threshold:
        t = np.nextafter(t, np.float32(np.inf))
    return float(t) if np.isfinite(t) else None


def check_edges_selection(top, threshold, max_edges):
    """the ValueErrors of the selection arguments of `effects_edges`"""
    if (top is None) == (threshold is None):
        raise ValueError("effects_edges: exactly one of `top` and `threshold` must be given")
    if top is not None and (not _is_int(top) or top < 1):
        raise ValueError("effects_edges: top must be an integer >= 1, got %r" % (top,))
    _check_threshold("effects_edges", threshold)
    if max_edges is not None:
        if threshold is None:
            raise ValueError("effects_edges: max_edges applies to `threshold` only")
        if not _is_int(max_edges) or not 1 <= max_edges < 2 ** 32:
            raise ValueError("effects_edges: max_edges must be an integer in [1, 2^32), got %r" % (max_edges,))


def effects_edges(params, mode, y=None, ph=None, top=None, threshold=None, orient=False, diagonal=False, max_edges=None,
                  refine_above=None):
    """phx_effects_edges on laid-out parameters (`Params`): the eligible entries (include/phoenix_hip.h) of the matrix
    `effects_matrix(params, mode, y, ph)` would return -- all with |M[i,j]| >= threshold, or the `top` strongest (ties at
    the cut to the smaller i, then j) -- as (regulator int64 [E], target int64 [E], value float32 [E]) on the device,
    sorted by magnitude descending, then i, then j.  The matrix is not formed: a COUNT pass (a histogram of the magnitude
    bits, read by the host) sizes the candidate list, at most one more refines the cut bin, an EMIT pass fills the list,
    and a sort of the candidates' 64-bit keys orders it.  `max_edges` (threshold only): no COUNT pass, one EMIT pass into
    a list of that capacity; RuntimeError with the true count when more entries qualify.  `refine_above`: the cap on the
    entries of the cut bin (default max(4 top, 2^20)): a fuller bin is refined once on its next 12 bits, and `top` raises
    RuntimeError when the refined cut bin is still fuller."""
    check_edges_selection(top, threshold, max_edges)
    y, ph, B = _effects_states("effects_edges", params, mode, y, ph, pairs=True)
    N, H, dev = params.N, params.H, params.device
    lib = _lib.load()
    nbytes = lib.phx_effects_edges_workspace_bytes(N, H, B, _lib.EFFECTS_MODES[mode])
    ws = _analysis_workspace(OP_EDGES, nbytes, dev).view(torch.int32)      # the histogram, then the cursor
    p = params.on_current_stream()
    flags = _edges_flags(orient, diagonal)

    def run(pass_, level=0, prefix=0, tau=0.0, keys=None, values=None):
        _check_call(lib.phx_effects_edges(C.byref(p.c), _lib.EFFECTS_MODES[mode], _p(y), _p(ph), B, flags, pass_, level,
                                          prefix, tau, _p(keys), _p(values), 0 if keys is None else keys.numel(), _p(ws),
                                          nbytes, _stream_ptr()))

    def histogram(level, prefix=0):
        run(_lib.EDGES_COUNT, level, prefix)
        return ws[:_lib.EDGES_BINS].cpu().numpy().astype(np.int64) & 0xFFFFFFFF    # the one small host read of the pass

    def empty():
        z = torch.empty(0, dtype=torch.int64, device=dev)
        return z, z.clone(), torch.empty(0, dtype=torch.float32, device=dev)

    if top is not None:
        K = int(top)
        cap = max(4 * K, EDGES_REFINE_MIN) if refine_above is None else int(refine_above)
        h = histogram(0)
        above = np.cumsum(h[::-1])[::-1]                    # above[b] = eligible entries in bins b ..
        if above[0] == 0:
            return empty()
        lo, cand = 1, int(above[0])                         # fewer than K eligible: all of them
        if above[0] > K:
            c = int(np.nonzero(above >= K)[0][-1])          # the cut bin
            lo, cand = c << 19, int(above[c])
            if h[c] > cap:
                h2 = histogram(1, c)
                assert int(h2.sum()) == int(h[c])
                above2 = np.cumsum(h2[::-1])[::-1] + (above[c] - h[c])
                c2 = int(np.nonzero(above2 >= K)[0][-1])
                if h2[c2] > cap:
                    raise RuntimeError("effects_edges: %d entries share the magnitude at the cut of top=%d (to 24 bits); "
                                       "the candidate list is capped at %d" % (int(h2[c2]), K, cap))
                lo, cand = (c << 19) | (c2 << 7), int(above2[c2])
        tau = float(np.uint32(max(lo, 1)).view(np.float32))
        capacity = cand
    else:
        K = None
        tau = _edges_tau(float(threshold))
        if tau is None:
            return empty()
        if max_edges is not None:
            capacity = int(max_edges)
        else:
            tb = _f32_bits(tau)
            c = tb >> 19
            h = histogram(0)
            capacity = int(h[c:].sum())
            if h[c] > (EDGES_REFINE_MIN if refine_above is None else int(refine_above)):    # the bin of tau itself is an upper bound: tighten it
                h2 = histogram(1, c)
                capacity = int(h[c + 1:].sum() + h2[(tb >> 7) & (_lib.EDGES_BINS - 1):].sum())
            if capacity == 0:
                return empty()
        if capacity >= 2 ** 32:
            raise ValueError("effects_edges: %d candidate edges do not fit one list" % capacity)
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    values = torch.empty(capacity, dtype=torch.float32, device=dev)
    run(_lib.EDGES_EMIT, tau=tau, keys=keys, values=values)
    n = int(ws[_lib.EDGES_BINS].item()) & 0xFFFFFFFF
    if n > capacity:
        if max_edges is not None:
            raise RuntimeError("effects_edges: %d edges qualify, max_edges=%d holds fewer; nothing is returned"
                               % (n, capacity))
        raise RuntimeError("effects_edges: the emit pass found %d entries where the count pass found %d" % (n, capacity))
    keys, order = torch.sort(keys[:n])
    if K is not None:
        keys, order = keys[:K], order[:K]
    flat = keys & 0xFFFFFFFF
    return torch.div(flat, N, rounding_mode="floor"), flat % N, values[order]


OP_NEIGHBORS = 9     # workspace-cache key of effects_neighbors (phx_effects_neighbors_workspace_bytes sizes it)


def _gene_set(name, what, x, N):
    """a candidate list (`regulators` / `targets` of `effects_neighbors`) as a one-dimensional int64 tensor on the device
    it came from, or None for all genes; ValueError for anything but integer gene indices inside [0, N)"""
    if x is None:
        return None
    try:
        x = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x if hasattr(x, "shape") else list(x)))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("%s: `%s` must be a sequence of gene indices" % (name, what))
    if x.numel() == 0:
        x = x.reshape(-1).to(torch.int64)
    if x.dim() != 1 or x.dtype == torch.bool or x.is_floating_point() or x.is_complex():
        raise ValueError("%s: `%s` must be a one-dimensional sequence of integer gene indices, got %s %s"
                         % (name, what, x.dtype, tuple(x.shape)))
    x = x.to(torch.int64)
    if x.numel() and (int(x.min()) < 0 or int(x.max()) >= N):
        raise ValueError("%s: `%s` must lie in [0, %d), got %d .. %d" % (name, what, N, int(x.min()), int(x.max())))
    return x


def _gene_masks(sets, N, device):
    """the candidate lists of `_gene_set` as byte masks [N] on the device (None stays None: every gene)"""
    masks = []
    for idx in sets:
        if idx is None:
            masks.append(None)
        else:
            m = torch.zeros(N, dtype=torch.uint8, device=device)
            m[idx.to(device)] = 1
            masks.append(m)
    return masks


def check_neighbors_selection(k, of, regulators, targets, threshold, N):
    """the ValueErrors of the selection arguments of `effects_neighbors`, raised before a device is needed: (k, axis,
    regulators, targets) with the candidate lists as int64 tensors or None"""
    name = "effects_neighbors"
    if not _is_int(k) or not 1 <= k <= _lib.NEIGHBORS_MAX_K:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (name, _lib.NEIGHBORS_MAX_K, k))
    if not isinstance(of, str) or of not in _lib.NEIGHBORS_AXES:
        raise ValueError('%s: of must be "target" or "regulator", got %r' % (name, of))
    _check_threshold(name, threshold)
    return int(k), _lib.NEIGHBORS_AXES[of], _gene_set(name, "regulators", regulators, N), _gene_set(name, "targets", targets, N)


def effects_neighbors(params, mode, k, of="target", y=None, ph=None, regulators=None, targets=None, threshold=None,
                      orient=False, diagonal=False):
    """phx_effects_neighbors on laid-out parameters (`Params`): for every line of the matrix `effects_matrix(params, mode, y,
    ph)` would return -- column n with of="target", row n with of="regulator" -- the k strongest eligible entries
    (include/phoenix_hip.h) as (gene int64 [N, k], value float32 [N, k], count int64 [N], strength float32 [N]) on the
    device.  `regulators` / `targets`: candidate gene indices (None: all), turned into byte masks on the device.  One call:
    the matrix is not formed."""
    k, axis, regulators, targets = check_neighbors_selection(k, of, regulators, targets, threshold, params.N)
    y, ph, B = _effects_states("effects_neighbors", params, mode, y, ph, pairs=True)
    N, H, dev = params.N, params.H, params.device
    tau = 0.0
    if threshold is not None:
        tau = _edges_tau(float(threshold))
        if tau is None:                                   # above every finite float32: nothing is eligible
            return (torch.full((N, k), -1, dtype=torch.int64, device=dev), torch.zeros((N, k), dtype=torch.float32, device=dev),
                    torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.float32, device=dev))
    masks = _gene_masks((regulators, targets), N, dev)
    lib = _lib.load()
    nbytes = lib.phx_effects_neighbors_workspace_bytes(N, H, B, _lib.EFFECTS_MODES[mode], axis, k)
    ws = _analysis_workspace(OP_NEIGHBORS, nbytes, dev)
    gene = torch.empty((N, k), dtype=torch.int32, device=dev)
    value = torch.empty((N, k), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    strength = torch.empty(N, dtype=torch.float32, device=dev)
    p = params.on_current_stream()
    _check_call(lib.phx_effects_neighbors(C.byref(p.c), _lib.EFFECTS_MODES[mode], _p(y), _p(ph), B,
                                          _edges_flags(orient, diagonal), axis, k, tau,
                                          _p(masks[0]), _p(masks[1]), _p(gene), _p(value), _p(count), _p(strength), _p(ws),
                                          nbytes, _stream_ptr()))
    return gene.to(torch.int64), value, count.to(torch.int64), strength


OP_APPLY = 14        # workspace-cache key of effects_apply (phx_effects_apply_workspace_bytes sizes it)


def check_apply_selection(name, of, weight, regulators, targets, threshold, N):
    """the ValueErrors of the selection arguments of `effects_apply` (and of the walks on it), raised before a device is
    needed: (axis, weight code, regulators, targets) with the candidate lists as int64 tensors or None"""
    if not isinstance(of, str) or of not in _lib.NEIGHBORS_AXES:
        raise ValueError('%s: of must be "target" or "regulator", got %r' % (name, of))
    if not isinstance(weight, str) or weight not in _lib.APPLY_WEIGHTS:
        raise ValueError('%s: weight must be "value", "abs" or "unit", got %r' % (name, weight))
    _check_threshold(name, threshold)
    return (_lib.NEIGHBORS_AXES[of], _lib.APPLY_WEIGHTS[weight], _gene_set(name, "regulators", regulators, N),
            _gene_set(name, "targets", targets, N))


def check_apply_block(name, v, N):
    """ValueError unless `v` is a tensor of shape [N] or [N, R] with R >= 1"""
    if not isinstance(v, torch.Tensor) or v.dim() not in (1, 2) or v.shape[0] != N or v.numel() == 0:
        raise ValueError("%s: v must be a tensor of shape [%d] or [%d, R] with R >= 1, got %s"
                         % (name, N, N, tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__))


class ApplyOperator:
    """The matrix `effects_matrix(params, mode, y, ph)` would return, filtered by the eligibility rules of
    `effects_neighbors` (include/phoenix_hip.h), as an operator on blocks of vectors: prepared once -- the states, the
    candidate masks and the threshold are checked and laid out here, with the host reads that takes -- and applied any
    number of times without a host synchronisation (phx_effects_apply; the matrix is never formed).  `regulators` and
    `targets` are what `_gene_set` returned."""

    def __init__(self, params, mode, y=None, ph=None, regulators=None, targets=None, threshold=None, orient=False,
                 diagonal=False, name="effects_apply"):
        _check_threshold(name, threshold)
        self.y, self.ph, self.B = _effects_states(name, params, mode, y, ph, pairs=True)
        self.params, self.mode, self.name = params, _lib.EFFECTS_MODES[mode], name
        self.tau = 0.0 if threshold is None else _edges_tau(float(threshold))     # None: above every finite float32
        self.masks = _gene_masks((regulators, targets), params.N, params.device)
        self.flags = _edges_flags(orient, diagonal)

    def apply(self, v, axis, weight):
        """out[n, r] = sum over the eligible entries of line n (column n of the matrix with axis "target", row n with
        "regulator") of w(entry) * v[other gene, r], w the entry ("value"), its magnitude ("abs") or 1 ("unit"): float32, of
        the shape of `v` ([N] or [N, R]).  Blocks of more than 32 columns are served 32 at a time."""
        N, H, dev = self.params.N, self.params.H, self.params.device
        check_apply_block(self.name, v, N)
        _require_f32(v, "v")
        if v.device != dev:
            raise ValueError("%s: v must be on the parameters' device" % self.name)
        axis = _lib.NEIGHBORS_AXES.get(axis, axis)
        weight = _lib.APPLY_WEIGHTS.get(weight, weight)
        v2 = v.detach().reshape(N, -1)
        R = v2.shape[1]
        if self.tau is None:                              # nothing is eligible
            return torch.zeros_like(v, dtype=torch.float32)
        lib = _lib.load()
        p = self.params.on_current_stream()
        out = torch.empty((N, R), dtype=torch.float32, device=dev)
        for c0 in range(0, R, _lib.APPLY_MAX_R):
            c1 = min(R, c0 + _lib.APPLY_MAX_R)
            whole = c0 == 0 and c1 == R
            vb = (v2 if whole else v2[:, c0:c1]).contiguous()
            ob = out if whole else torch.empty((N, c1 - c0), dtype=torch.float32, device=dev)
            nbytes = lib.phx_effects_apply_workspace_bytes(N, H, self.B, self.mode, axis, c1 - c0)
            ws = _analysis_workspace(OP_APPLY, nbytes, dev)
            _check_call(lib.phx_effects_apply(C.byref(p.c), self.mode, _p(self.y), _p(self.ph), self.B, self.flags, axis,
                                              weight, self.tau, _p(self.masks[0]), _p(self.masks[1]), _p(vb), c1 - c0,
                                              _p(ob), _p(ws), nbytes, _stream_ptr()))
            if not whole:
                out[:, c0:c1] = ob
        return out.reshape(v.shape)


def effects_apply(params, mode, v, of="target", weight="value", y=None, ph=None, regulators=None, targets=None, threshold=None,
                  orient=False, diagonal=False):
    """phx_effects_apply on laid-out parameters (`Params`): the product of the block `v` ([N] or [N, R] float32 on the
    device) with the eligible entries of the matrix `effects_matrix(params, mode, y, ph)` would return, along its columns
    (of="target": M^T v) or its rows (of="regulator": M v); see `ApplyOperator`."""
    axis, weight, regulators, targets = check_apply_selection("effects_apply", of, weight, regulators, targets, threshold,
                                                              params.N)
    check_apply_block("effects_apply", v, params.N)
    op = ApplyOperator(params, mode, y=y, ph=ph, regulators=regulators, targets=targets, threshold=threshold, orient=orient,
                       diagonal=diagonal)
    return op.apply(v, axis, weight)


OP_PATHWAYS = 10     # workspace-cache key of pathway_permutations (phx_pathway_permutations_workspace_bytes sizes it)


def check_permutation_range(name, seed, first, n_perm):
    """the ValueErrors of (seed, first, n_perm) of `pathway_permutations`, raised before a device is needed"""
    if not _is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError("%s: seed must be an integer in [0, 2^64), got %r" % (name, seed))
    if not _is_int(first) or first < 0:
        raise ValueError("%s: first must be an integer >= 0, got %r" % (name, first))
    if not _is_int(n_perm) or n_perm < 1:
        raise ValueError("%s: n_perm must be an integer >= 1, got %r" % (name, n_perm))
    if first + n_perm > _lib.PATHWAYS_MAX_R:
        raise ValueError("%s: first + n_perm must not exceed 2^50, got %d + %d" % (name, first, n_perm))
    return int(seed), int(first), int(n_perm)


def pathway_permutations(scores, ptr, idx, seed, first, n_perm):
    """phx_pathway_permutations (include/phoenix_hip.h): `scores` float32 [N], N <= 16384, and the P pathways in CSR form,
    `ptr` int64 [P + 1] and `idx` int32 or int64 [nnz] (member genes, unique within a pathway), all on one device.  Returns
    the raw results of the permutations [first, first + n_perm) of `seed` on that device: (base float64 [P], count int64
    [P], s1 float64 [P], s2 float64 [P]).  ValueError for anything the kernel would trust: a `ptr` that is not a CSR
    pointer of `idx`, a member outside [0, N) or repeated in its pathway, a score that is not finite.  The pathways go to
    the kernel sorted by size (the lanes of a wave then walk lists of similar length) and the results come back in the
    caller's order; a pathway's own member order, which fixes the order of its sums, is kept."""
    name = "pathway_permutations"
    seed, first, n_perm = check_permutation_range(name, seed, first, n_perm)
    for what, x in (("scores", scores), ("ptr", ptr), ("idx", idx)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s: `%s` must be a tensor on the GPU, got %s" % (name, what, type(x).__name__))
        _require_gpu(x, what)
    dev = scores.device
    if ptr.device != dev or idx.device != dev:
        raise ValueError("%s: scores, ptr and idx must be on one device" % name)
    if scores.dim() != 1 or not 1 <= scores.shape[0] <= _lib.PATHWAYS_MAX_N:
        raise ValueError("%s: scores must be [N] with 1 <= N <= %d, got %s" % (name, _lib.PATHWAYS_MAX_N, tuple(scores.shape)))
    if ptr.dim() != 1 or ptr.dtype != torch.int64 or ptr.shape[0] < 2:
        raise ValueError("%s: ptr must be int64 [P + 1] with P >= 1, got %s %s" % (name, ptr.dtype, tuple(ptr.shape)))
    if idx.dim() != 1 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: idx must be int32 or int64 [nnz], got %s %s" % (name, idx.dtype, tuple(idx.shape)))
    N, P, nnz = scores.shape[0], ptr.shape[0] - 1, idx.shape[0]
    if P >= 2 ** 31:
        raise ValueError("%s: at most 2^31 - 1 pathways, got %d" % (name, P))
    scores, ptr, idx = scores.detach().contiguous(), ptr.contiguous(), idx.contiguous()
    sizes = ptr[1:] - ptr[:-1]
    if int(ptr[0]) != 0 or int(ptr[-1]) != nnz or (P and int(sizes.min()) < 0):
        raise ValueError("%s: ptr must start at 0, not decrease and end at len(idx) = %d" % (name, nnz))
    if nnz and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError("%s: idx must lie in [0, %d), got %d .. %d" % (name, N, int(idx.min()), int(idx.max())))
    owner = torch.repeat_interleave(torch.arange(P, device=dev), sizes)
    if nnz and int(torch.unique(owner * N + idx).numel()) != nnz:
        raise ValueError("%s: a pathway lists a gene more than once" % name)
    if not bool(torch.isfinite(scores).all()):
        raise ValueError("%s: scores must be finite" % name)
    # by size, largest first, stably: the pathways move as blocks, their members stay in order
    order = torch.sort(sizes, descending=True, stable=True).indices
    s_sizes = sizes[order]
    s_ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    torch.cumsum(s_sizes, 0, out=s_ptr[1:])
    within = torch.arange(nnz, device=dev) - torch.repeat_interleave(s_ptr[:-1], s_sizes)
    s_idx = idx[torch.repeat_interleave(ptr[:-1][order], s_sizes) + within].to(torch.int32)
    lib = _lib.load()
    nbytes = lib.phx_pathway_permutations_workspace_bytes(N, P, nnz, n_perm)
    ws = _analysis_workspace(OP_PATHWAYS, nbytes, dev)
    base = torch.empty(P, dtype=torch.float64, device=dev)
    count = torch.empty(P, dtype=torch.int64, device=dev)
    s1 = torch.empty(P, dtype=torch.float64, device=dev)
    s2 = torch.empty(P, dtype=torch.float64, device=dev)
    _check_call(lib.phx_pathway_permutations(_p(scores), N, _p(s_ptr), _p(s_idx), P, nnz, seed, first, n_perm, _p(base), _p(count),
                                             _p(s1), _p(s2), _p(ws), nbytes, _stream_ptr()))
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(P, device=dev)
    return base[inverse], count[inverse], s1[inverse], s2[inverse]


OP_NETSCORE = 8      # workspace-cache key of network_score (phx_effects_rank_workspace_bytes sizes it)
NETSCORE_TILE = 64  # the tile by which phx_effects_gather wants its keys grouped


def check_network_indices(name, regulator, target, N):
    """(regulator, target) of a label set as int64 tensors [E], each on the device it came from (the host for lists and
    numpy arrays); ValueError for arrays of unequal length, of a non-integer dtype or with an index outside [0, N)"""
    out = []
    for what, x in (("regulator", regulator), ("target", target)):
        try:
            x = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("%s: `%s` must be an array of gene indices" % (name, what))
        if x.numel() == 0:
            x = x.to(torch.int64)
        if x.dim() != 1 or x.dtype in (torch.bool,) or x.is_floating_point() or x.is_complex():
            raise ValueError("%s: `%s` must be a one-dimensional array of integer gene indices, got %s %s"
                             % (name, what, x.dtype, tuple(x.shape)))
        out.append(x.to(torch.int64))
    r, t = out
    if r.numel() != t.numel():
        raise ValueError("%s: regulator and target must have the same length, got %d and %d" % (name, r.numel(), t.numel()))
    if r.numel():
        lo, hi = min(int(r.min()), int(t.min())), max(int(r.max()), int(t.max()))
        if lo < 0 or hi >= N:
            raise ValueError("%s: gene indices must lie in [0, %d), got %d .. %d" % (name, N, lo, hi))
    return r, t


def _u32(x):
    """an int64 tensor of values in [0, 2^32) as the int32 tensor with the same low 32 bits (what the kernels read as
    unsigned)"""
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def effects_gather(params, mode, regulator, target, y=None, ph=None, orient=False):
    """phx_effects_gather on laid-out parameters (`Params`): float32 [E] on the device, element e the entry (regulator[e],
    target[e]) of the matrix `effects_matrix(params, mode, y, ph)` would return, bit for bit, or with `orient` of its
    make_mask form (include/phoenix_hip.h).  regulator, target: int64 tensors [E] on the parameters' device with values in
    [0, N) (check_network_indices); duplicates are allowed.  The keys are grouped by tile with one sort; only the tiles
    that hold a listed entry are formed."""
    y, ph, B = _effects_states("effects_at", params, mode, y, ph, pairs=True)
    N, dev = params.N, params.device
    E = regulator.numel()
    if E == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    if E >= 2 ** 32:
        raise ValueError("effects_at: %d entries do not fit one list" % E)
    T = (N + NETSCORE_TILE - 1) // NETSCORE_TILE
    tile = torch.div(regulator, NETSCORE_TILE, rounding_mode="floor") * T + torch.div(target, NETSCORE_TILE, rounding_mode="floor")
    tile, order = torch.sort(tile)
    keys = _u32((regulator * N + target)[order])
    bounds = torch.arange(T * T + 1, dtype=torch.int64, device=dev)
    offsets = _u32(torch.searchsorted(tile, bounds))
    sorted_values = torch.empty(E, dtype=torch.float32, device=dev)
    p = params.on_current_stream()
    _check_call(_lib.load().phx_effects_gather(C.byref(p.c), _lib.EFFECTS_MODES[mode], _p(y), _p(ph), B,
                                               _edges_flags(orient, False), _p(keys), _p(offsets), E, _p(sorted_values),
                                               _stream_ptr()))
    values = torch.empty_like(sorted_values)
    values[order] = sorted_values
    return values


def network_score(params, mode, regulator, target, y=None, ph=None, orient=False, diagonal=False):
    """The rank statistics of the matrix `effects_matrix(params, mode, y, ph)` (with `orient`: of its make_mask form)
    against the label set (regulator, target) -- int64 tensors [E] on the parameters' device with values in [0, N) -- without
    the matrix: (auroc, average_precision, n_positive, n_negative, threshold float32 [m], tp int64 [m], fp int64 [m]),
    the three arrays on the device (include/phoenix_hip.h: phx_effects_gather, phx_effects_rank_counts).  GATHER reads the
    positives' values, a sort makes the distinct magnitudes u and their multiplicities, RANK counts every scored entry
    between and on them, and cumulative sums of the 2 m + 1 counts are the curve.  Everything is integer arithmetic up to
    the two final float64 divisions."""
    y, ph, B = _effects_states("network_score", params, mode, y, ph, pairs=True)
    N, dev = params.N, params.device
    key = torch.unique(regulator * N + target)
    if not diagonal:
        key = key[key % (N + 1) != 0]                 # i N + i = i (N + 1)
    n_scored = N * N - (0 if diagonal else N)
    P = int(key.numel())
    Nn = n_scored - P
    if P == 0 or Nn == 0:
        raise ValueError("network_score: Only one class present in the labels (%d positives, %d negatives); the scores "
                         "are not defined in that case" % (P, Nn))
    reg = torch.div(key, N, rounding_mode="floor")
    values = effects_gather(params, mode, reg, key - reg * N, y=y, ph=ph, orient=orient)
    mag = values.view(torch.int32) & 0x7FFFFFFF
    u, mult = torch.unique(mag, return_counts=True)   # ascending
    m = int(u.numel())
    lib = _lib.load()
    nbytes = lib.phx_effects_rank_workspace_bytes(N, params.H, B, _lib.EFFECTS_MODES[mode])
    ws = _analysis_workspace(OP_NETSCORE, nbytes, dev).view(torch.int32)    # the count of non-finite entries first
    counts = torch.empty(2 * m + 1, dtype=torch.int32, device=dev)
    p = params.on_current_stream()
    _check_call(lib.phx_effects_rank_counts(C.byref(p.c), _lib.EFFECTS_MODES[mode], _p(y), _p(ph), B,
                                            _edges_flags(orient, diagonal), _p(u), m, _p(counts), _p(ws), nbytes,
                                            _stream_ptr()))
    bad = int(ws[0].item()) & 0xFFFFFFFF
    if bad:
        raise ValueError("network_score: %d scored entries are not finite" % bad)
    c = counts.to(torch.int64) & 0xFFFFFFFF
    if int(c.sum()) != n_scored:
        raise RuntimeError("network_score: the rank pass counted %d entries of %d" % (int(c.sum()), n_scored))
    # descending thresholds: everything at or above u[k] is the buckets 2 k + 1 ..
    at, between = c[1::2], c[0::2]                    # at[k] ties with u[k]; between[k] lies below u[k] (between[m]: above all)
    ge_all = torch.flip(torch.cumsum(torch.flip(at + between[1:], (0,)), 0), (0,))      # entries >= u[k]
    ge_pos = torch.flip(torch.cumsum(torch.flip(mult, (0,)), 0), (0,))                  # positives >= u[k]
    gt_pos = ge_pos - mult
    # U2 = sum over all scored entries of (2 gt + eq) - P^2:  an entry tied with u[k] has gt = gt_pos[k], eq = mult[k]; one
    # in the gap below u[k] has gt = ge_pos[k], eq = 0; one above all positives has neither
    U2 = int((at * (2 * gt_pos + mult)).sum() + (between[:m] * (2 * ge_pos)).sum()) - P * P
    auroc = U2 / (2 * P * Nn)
    tp = torch.flip(ge_pos, (0,))
    fp = torch.flip(ge_all, (0,)) - tp
    hits = torch.flip(mult, (0,)).to(torch.float64)   # tp[k] - tp[k - 1]
    ap = float((hits / P * (tp.to(torch.float64) / (tp + fp).to(torch.float64))).sum())
    threshold = torch.flip(u, (0,)).view(torch.float32)
    return auroc, ap, P, Nn, threshold, tp, fp


OP_REDUCED_JACOBIAN = 15   # workspace-cache key of reduced_jacobian (phx_reduced_jacobian_workspace_bytes sizes it)
OP_STEADY_SOLVE = 16       # ... and of steady_solve (phx_steady_solve_workspace_bytes)


def _steady_rows(name, p, x, what="y"):
    """`x` as contiguous float32 [B, N] rows on the parameters' device"""
    _require_gpu(x, what)
    if x.dim() != 2 or x.shape[1] != p.N or x.shape[0] < 1:
        raise ValueError("%s: %s must be [B, %d], got %s" % (name, what, p.N, tuple(x.shape)))
    return x.detach().contiguous()


def reduced_jacobian(p, y, m, r=None):
    """phx_reduced_jacobian on laid-out parameters (`Params`): for the states y [B, N] and the per-gene weights m [B, N]
    (float32; exact 0: the gene takes no part) returns (S [B, 2H, 2H], w [B, 2H] or None, hid [B, 2H]) with
    S_b = C(y_b) diag(m_b) Wa, w_b = C(y_b) (m_b r_b) where `r` [B, N] is given, and the hidden vector of y_b."""
    y2 = _steady_rows("reduced_jacobian", p, y)
    m2 = _steady_rows("reduced_jacobian", p, m, "m")
    r2 = None if r is None else _steady_rows("reduced_jacobian", p, r, "r")
    if m2.shape != y2.shape or (r2 is not None and r2.shape != y2.shape):
        raise ValueError("reduced_jacobian: y, m and r must have one shape")
    B, H2, dev = y2.shape[0], 2 * p.H, y2.device
    S = torch.empty((B, H2, H2), dtype=torch.float32, device=dev)
    hid = torch.empty((B, H2), dtype=torch.float32, device=dev)
    w = None if r2 is None else torch.empty((B, H2), dtype=torch.float32, device=dev)
    p.on_current_stream()
    nbytes = _ws_size((OP_REDUCED_JACOBIAN, p.N, p.H, B), "phx_reduced_jacobian_workspace_bytes", p.N, p.H, B)
    ws = _analysis_workspace(OP_REDUCED_JACOBIAN, nbytes, dev)
    _check_call(_lib.load().phx_reduced_jacobian(C.byref(p.c), _p(y2), _p(m2), _p(r2), B, _p(S), _p(w), _p(hid), _p(ws), nbytes,
                                                 _stream_ptr()))
    return S, w, hid


def steady_residual(p, y):
    """(hid [B, 2H], r [B, N] = Wa hid - y) of the states y [B, N]: phx_steady_residual"""
    y2 = _steady_rows("steady_residual", p, y)
    hid = torch.empty((y2.shape[0], 2 * p.H), dtype=torch.float32, device=y2.device)
    r = torch.empty_like(y2)
    p.on_current_stream()
    _check_call(_lib.load().phx_steady_residual(C.byref(p.c), _p(y2), y2.shape[0], _p(hid), _p(r), _stream_ptr()))
    return hid, r


def steady_update(p, y, m, r, x):
    """y + m (r + Wa x) where m != 0, y where m == 0: phx_steady_update (all contiguous float32 on the device)"""
    out = torch.empty_like(y)
    p.on_current_stream()
    _check_call(_lib.load().phx_steady_update(C.byref(p.c), _p(y), _p(m), _p(r), _p(x), y.shape[0], _p(out), _stream_ptr()))
    return out


def steady_solve(S, w):
    """(x [B, n] float32, info [B] int32) of (I - S_b) x_b = w_b, solved in float64 on the device: phx_steady_solve.  S
    [B, n, n] and w [B, n] float32 on one device, n even; a view (a transpose, say) is solved as the matrix it shows."""
    _require_gpu(S, "S")
    _require_gpu(w, "w")
    if S.dim() != 3 or S.shape[1] != S.shape[2] or S.shape[1] % 2 or S.shape[0] < 1:
        raise ValueError("steady_solve: S must be [B, 2H, 2H], got %s" % (tuple(S.shape),))
    if tuple(w.shape) != tuple(S.shape[:2]) or w.device != S.device:
        raise ValueError("steady_solve: w must be %s on the device of S, got %s" % (tuple(S.shape[:2]), tuple(w.shape)))
    S, w = S.detach().contiguous(), w.detach().contiguous()
    B, n = w.shape
    x = torch.empty_like(w)
    info = torch.empty(B, dtype=torch.int32, device=w.device)
    nbytes = _ws_size((OP_STEADY_SOLVE, n, B), "phx_steady_solve_workspace_bytes", n // 2, B)
    ws = _analysis_workspace(OP_STEADY_SOLVE, nbytes, w.device)
    _check_call(_lib.load().phx_steady_solve(_p(S), _p(w), n // 2, B, _p(x), _p(info), _p(ws), nbytes, _stream_ptr()))
    return x, info


OP_STEADY_PROJECT = 17     # workspace-cache key of steady_adjoint_project (phx_steady_adjoint_project_workspace_bytes)
OP_STEADY_PGRADS = 18      # ... and of steady_param_grads (phx_steady_param_grads_workspace_bytes)


def _steady_hidden(name, p, x, B, what):
    """`x` as contiguous float32 [B, 2H] on the device"""
    _require_gpu(x, what)
    if tuple(x.shape) != (B, 2 * p.H):
        raise ValueError("%s: %s must be [%d, %d], got %s" % (name, what, B, 2 * p.H, tuple(x.shape)))
    return x.detach().contiguous()


def steady_adjoint_project(p, m, gy):
    """b [B, 2H] = WaT (m gy) of the cotangents gy [B, N] and the weights m [B, N] (exact 0: the gene is not read):
    phx_steady_adjoint_project"""
    m2 = _steady_rows("steady_adjoint_project", p, m, "m")
    g2 = _steady_rows("steady_adjoint_project", p, gy, "gy")
    if m2.shape != g2.shape:
        raise ValueError("steady_adjoint_project: m and gy must have one shape")
    B, dev = m2.shape[0], m2.device
    b = torch.empty((B, 2 * p.H), dtype=torch.float32, device=dev)
    p.on_current_stream()
    nbytes = _ws_size((OP_STEADY_PROJECT, p.N, p.H, B), "phx_steady_adjoint_project_workspace_bytes", p.N, p.H, B)
    ws = _analysis_workspace(OP_STEADY_PROJECT, nbytes, dev)
    _check_call(_lib.load().phx_steady_adjoint_project(C.byref(p.c), _p(m2), _p(g2), B, _p(b), _p(ws), nbytes, _stream_ptr()))
    return b


def steady_adjoint_back(p, y, m, gy, q, hid):
    """(lam [B, N] = m (gy + C(y)^T q), gy0 [B, N] = (1 - m) (gy + C(y)^T q)) with q, hid [B, 2H]: phx_steady_adjoint_back"""
    name = "steady_adjoint_back"
    y2, m2, g2 = _steady_rows(name, p, y), _steady_rows(name, p, m, "m"), _steady_rows(name, p, gy, "gy")
    if m2.shape != y2.shape or g2.shape != y2.shape:
        raise ValueError("%s: y, m and gy must have one shape" % name)
    B = y2.shape[0]
    q2, h2 = _steady_hidden(name, p, q, B, "q"), _steady_hidden(name, p, hid, B, "hid")
    lam, gy0 = torch.empty_like(y2), torch.empty_like(y2)
    p.on_current_stream()
    _check_call(_lib.load().phx_steady_adjoint_back(C.byref(p.c), _p(y2), _p(m2), _p(g2), _p(q2), _p(h2), B, _p(lam), _p(gy0),
                                                    _stream_ptr()))
    return lam, gy0


def steady_param_grads(p, y, lam, q, hid, grads=None):
    """phx_steady_param_grads: the parameter gradients of the rows y, lam [B, N], q, hid [B, 2H] as `Grads`.  `grads`: a
    `Grads` of an earlier call (of another block of rows) to add to; None: a fresh one, written."""
    name = "steady_param_grads"
    y2, l2 = _steady_rows(name, p, y), _steady_rows(name, p, lam, "lam")
    if l2.shape != y2.shape:
        raise ValueError("%s: y and lam must have one shape" % name)
    B, dev = y2.shape[0], y2.device
    q2, h2 = _steady_hidden(name, p, q, B, "q"), _steady_hidden(name, p, hid, B, "hid")
    if grads is None:
        grads = p.new_grads()
    else:
        grads.c.overwrite = 0
    p.on_current_stream()
    nbytes = _ws_size((OP_STEADY_PGRADS, p.N, p.H, B), "phx_steady_param_grads_workspace_bytes", p.N, p.H, B)
    ws = _analysis_workspace(OP_STEADY_PGRADS, nbytes, dev)
    _check_call(_lib.load().phx_steady_param_grads(C.byref(p.c), _p(y2), _p(l2), _p(q2), _p(h2), B, C.byref(grads.c), _p(ws), nbytes,
                                                   _stream_ptr()))
    return grads


OP_STEADY_INVERSE = 19     # workspace-cache key of steady_inverse (phx_steady_inverse_workspace_bytes)
RESPONSE_INPUTS = {"production": 0, "level": 1}       # phx_steady_response_factors / phx_steady_response: input


def steady_inverse(S):
    """(Z [B, n, n] float32 = (I - S_b)^-1 computed in float64 on the device, info [B] int32 -- phx_steady_solve's codes; Z_b = 0
    where info[b] != 0): phx_steady_inverse"""
    _require_gpu(S, "S")
    if S.dim() != 3 or S.shape[1] != S.shape[2] or S.shape[1] % 2 or S.shape[0] < 1:
        raise ValueError("steady_inverse: S must be [B, 2H, 2H], got %s" % (tuple(S.shape),))
    S = S.detach().contiguous()
    B, n = S.shape[0], S.shape[1]
    Z = torch.empty_like(S)
    info = torch.empty(B, dtype=torch.int32, device=S.device)
    nbytes = _ws_size((OP_STEADY_INVERSE, n, B), "phx_steady_inverse_workspace_bytes", n // 2, B)
    ws = _analysis_workspace(OP_STEADY_INVERSE, nbytes, S.device)
    _check_call(_lib.load().phx_steady_inverse(_p(S), n // 2, B, _p(Z), _p(info), _p(ws), nbytes, _stream_ptr()))
    return Z, info


def _response_genes(name, p, genes):
    _require_gpu(genes, "genes")
    if genes.dtype != torch.int32 or genes.dim() != 1 or genes.numel() < 1:
        raise ValueError("%s: genes must be a non-empty int32 vector on the device" % name)
    return genes.contiguous()


def steady_response_factors(p, y, m, hid, Z, info, genes, input):
    """(X [B, 2H, K], use [B, K]) of phx_steady_response_factors: the columns Z_b C_b[:, genes[k]], scaled by m_bk
    (input "production") or 1 / d_bk ("level"); a column of a row with info != 0 or a d that is 0 or not finite is 0, use 0.
    genes: int32 [K] on the device, every entry one of 0 .. N - 1 (the caller has checked them on the host)."""
    name = "steady_response_factors"
    y2, m2 = _steady_rows(name, p, y), _steady_rows(name, p, m, "m")
    B, H2, dev = y2.shape[0], 2 * p.H, y2.device
    if m2.shape != y2.shape or tuple(Z.shape) != (B, H2, H2) or tuple(info.shape) != (B,) or info.dtype != torch.int32:
        raise ValueError("%s: y, m [B, N], Z [B, 2H, 2H] and info [B] int32 do not go together" % name)
    h2 = _steady_hidden(name, p, hid, B, "hid")
    _require_gpu(Z, "Z")
    g = _response_genes(name, p, genes)
    K = g.numel()
    X = torch.empty((B, H2, K), dtype=torch.float32, device=dev)
    use = torch.empty((B, K), dtype=torch.float32, device=dev)
    p.on_current_stream()
    _check_call(_lib.load().phx_steady_response_factors(C.byref(p.c), _p(y2), _p(m2), _p(h2), _p(Z.detach().contiguous()),
                                                        _p(info.contiguous()), B, _p(g), K, RESPONSE_INPUTS[input], _p(X), _p(use),
                                                        _stream_ptr()))
    return X, use


def steady_response(p, m, X, use, genes, input, mean_abs, out=None):
    """phx_steady_response: out [K, N], the mean over the used states of m_bj sum_c WaT[c, j] X_b[c, k] (of its absolute value
    where mean_abs), with the diagonal of the input (see the header).  out: a [K, N] float32 view with contiguous rows (a
    block of rows of a larger matrix) to write into; None: a new tensor."""
    name = "steady_response"
    m2 = _steady_rows(name, p, m, "m")
    g = _response_genes(name, p, genes)
    B, K = m2.shape[0], g.numel()
    if tuple(X.shape) != (B, 2 * p.H, K) or tuple(use.shape) != (B, K) or not X.is_contiguous() or not use.is_contiguous():
        raise ValueError("%s: X must be contiguous [%d, %d, %d] and use [%d, %d]" % (name, B, 2 * p.H, K, B, K))
    if out is None:
        out = torch.empty((K, p.N), dtype=torch.float32, device=m2.device)
    if tuple(out.shape) != (K, p.N) or out.dtype != torch.float32 or out.stride(1) != 1 or out.stride(0) < p.N or not out.is_cuda:
        raise ValueError("%s: out must be float32 [%d, %d] with contiguous rows on the device" % (name, K, p.N))
    p.on_current_stream()
    _check_call(_lib.load().phx_steady_response(C.byref(p.c), _p(m2), _p(X), _p(use), B, _p(g), K, RESPONSE_INPUTS[input],
                                                1 if mean_abs else 0, _p(out), out.stride(0), _stream_ptr()))
    return out
