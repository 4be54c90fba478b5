"""The reference's `training_step` (ode_net/code/train_insilico.py:124-140, = train_breast.py:161-187)
on the engine: same inputs, same two losses, same composed gradient, same optimizer step -- but the
B per-sample `odeint_adjoint` calls are one launch and the prior branch runs on the HIP RHS kernels."""
import torch

from . import engine
from .odeint import _check_inputs, _out_shape, _prepare, odeint_adjoint, odeint_calls


def training_step(odenet, data_handler, opt, method, batch_size, explicit_time, relative_error, batch_for_prior,
                  prior_grad, loss_lambda, grad_sync=None):
    """`grad_sync`: optional callable run between backward() and opt.step() (data-parallel all-reduce,
    phoenix_amd.parallel.allreduce_grads, or a phoenix_amd.parallel.GradSync, which also makes every rank fail
    together when one rank's solve fails); everything else is the reference signature."""
    batch, t, target = data_handler.get_batch(batch_size)            # [B,1,N], [B,2], [B,1,N]
    opt.zero_grad()
    failure = None
    # Data-parallel shards of unequal size: the reference's losses are means over the WHOLE batch (train_insilico.py:132,136),
    # so a rank's local means enter with B_local / B_global and K_local / K_global and the gradients are summed.  Asked
    # before the solve: a count collective (GradSync(weighted=True)) must be met by every rank, also one whose solve fails.
    wd = wp = 1.0
    if grad_sync is not None and hasattr(grad_sync, "loss_weights"):
        wd, wp = grad_sync.loss_weights(batch.shape[0], batch_for_prior.shape[0], batch.device)
    overlap = bool(getattr(grad_sync, "overlap", False))
    issued = [0]          # gradient collectives the overlapped path has started (a failing rank tops them up below)
    try:
        # reference: python loop of odeint(odenet, batch_point, time)[1]; here one launch, per-sample control
        predictions = odeint_adjoint(odenet, batch, t, method=method)[1]
        loss_data = torch.mean((predictions - target) ** 2)
        if hasattr(odenet, "prior_mse"):     # phoenix_amd.ODENet: fused on the engine (no [K,1,N] prediction tensor)
            loss_prior = odenet.prior_mse(t, batch_for_prior, prior_grad)
        else:                                # the reference's own ODENet class
            pred_grad = odenet.prior_only_forward(t, batch_for_prior)
            loss_prior = torch.mean((pred_grad - prior_grad) ** 2)
        if overlap:
            _backward_overlapped(odenet, grad_sync, loss_lambda * loss_data if wd == 1.0 else (loss_lambda * wd) * loss_data,
                                 (1 - loss_lambda) * loss_prior if wp == 1.0 else ((1 - loss_lambda) * wp) * loss_prior,
                                 issued)
        elif wd == 1.0 and wp == 1.0:
            composed_loss = loss_lambda * loss_data + (1 - loss_lambda) * loss_prior
            composed_loss.backward()
        else:
            composed_loss = (loss_lambda * wd) * loss_data + ((1 - loss_lambda) * wp) * loss_prior
            composed_loss.backward()
    except (AssertionError, RuntimeError) as err:   # a failed solve (the reference's asserts, rk_common.py:174-176) or launch
        if not getattr(grad_sync, "collective_errors", False):
            raise
        failure = err                        # the other ranks are on their way into the collective: meet them there
    if grad_sync is not None:
        if overlap:
            # every rank issues the same sequence of collectives: a rank whose step failed part-way sends zeros for the
            # gradient reductions it did not reach (the flag below then stops every rank in this step)
            while failure is not None and issued[0] < 2:
                h = grad_sync.reduce_async([torch.zeros_like(p) for p in odenet.parameters() if p.requires_grad])
                issued[0] += 1
                if h is not None:
                    h.wait()
            grad_sync(odenet, error=failure, reduced=True)
        elif failure is not None:
            grad_sync(odenet, error=failure)
        else:
            grad_sync(odenet)
    opt.step()
    return [loss_data, loss_prior]


def _backward_overlapped(odenet, grad_sync, term_data, term_prior, issued):
    """The two loss terms are differentiated separately into separate gradient buffers: the all-reduce of the data-loss
    gradients (ready once the backward solve and its reduction kernel have run) is in flight while the prior branch's
    backward chain computes; both sets are summed over the ranks, then added into `.grad`.  The persistent solve kernels
    never share the device with the collective: the next step's forward solve is ordered behind both waits."""
    params = [p for p in odenet.parameters() if p.requires_grad]
    g_data = torch.autograd.grad(term_data, params, allow_unused=True)
    g_data = [g.contiguous() if g is not None else torch.zeros_like(p) for g, p in zip(g_data, params)]
    h_data = grad_sync.reduce_async(g_data)
    issued[0] += 1
    g_prior = torch.autograd.grad(term_prior, params, allow_unused=True)
    g_prior = [g.contiguous() if g is not None else torch.zeros_like(p) for g, p in zip(g_prior, params)]
    h_prior = grad_sync.reduce_async(g_prior)
    issued[0] += 1
    for h in (h_data, h_prior):
        if h is not None:
            h.wait()
    scale = getattr(grad_sync, "scale", None)
    for p, a, b in zip(params, g_data, g_prior):
        a.add_(b)
        if scale is not None:
            a.mul_(scale)
        p.grad = a


def _validation_pairs(odenet, data_handler, method):
    """(predictions, targets) of the reference's validation loop (train_insilico.py:77-101), rows in its order.
    Per item: the NaN times and the rows that go with them are dropped, the surviving rows `batch_point[idx[:-1]]` are ONE
    odeint call (one step controller shared by the rows) over the item's surviving times, and output 1 of every row is
    kept -- row i started at time[0] and read at time[1] is compared with target[i], exactly as the reference does it.
    Items with the same number of surviving rows are one `odeint_calls` with a time grid per call.  Output 1 depends on
    the first interval only (adaptive steps are not clipped to later output times, fixed grids step interval by
    interval: tests/test_validation_cpu.py shows it on the oracle), so a call gets time[:2]."""
    data, t, target_full, _n_val = data_handler.get_validation_set()
    if not torch.is_tensor(t) or t.shape[0] == 0:
        raise ValueError("phoenix_amd.validation: the data handler has no validation set")
    N = data.shape[-1]
    K = t.shape[0]
    ok = (~torch.isnan(t)).cpu().numpy()                      # the one host read: which times exist
    data = data.reshape(K, -1, N)                             # [K, rows, N]: `single` has one row per item
    target_full = target_full.reshape(K, -1, N)
    keep = []                                                 # per item: (surviving time indices, row indices)
    for k in range(K):
        idx = [i for i in range(ok.shape[1]) if ok[k, i]]
        if len(idx) < 2:
            raise IndexError("phoenix_amd.validation: validation item %d has fewer than two time points" % k)
        keep.append((idx, idx[:-1]))
    groups = {}
    for k, (_, rows) in enumerate(keep):
        groups.setdefault(len(rows), []).append(k)
    dev = data.device
    offs, total = [], 0
    for _, rows in keep:
        offs.append(total)
        total += len(rows)
    predictions = torch.empty((total, N), dtype=data.dtype, device=dev)
    targets = torch.empty((total, N), dtype=target_full.dtype, device=dev)
    for nrows, items in sorted(groups.items()):
        ki = torch.as_tensor([k for k in items for _ in range(nrows)], device=dev)
        ri = torch.as_tensor([r for k in items for r in keep[k][1]], device=dev)
        ti = torch.as_tensor([keep[k][0][:2] for k in items], device=dev)
        y0s = data[ki, ri].reshape(len(items), nrows, 1, N)
        grids = t[torch.as_tensor(items, device=dev)].gather(1, ti)          # [calls, 2]
        out = odeint_calls(odenet, y0s, grids, method=method)[:, 1]          # [calls, rows, 1, N]
        dst = torch.as_tensor([offs[k] + j for k in items for j in range(nrows)], device=dev)
        predictions.index_copy_(0, dst, out.reshape(-1, N).to(predictions.dtype))
        targets.index_copy_(0, dst, target_full[ki, ri])
    return predictions, targets


def validation(odenet, data_handler, method, explicit_time):
    """The reference's `validation` (train_insilico.py:77-106): [mean squared error over the validation set, n_val].
    One launch per group of items with equally many surviving time points instead of one per item."""
    with torch.no_grad():
        predictions, targets = _validation_pairs(odenet, data_handler, method)
        loss = torch.mean((predictions - targets) ** 2)
    return [loss, data_handler.n_val]


def my_r_squared(output, target):
    """train_insilico.py:43-49: squared Pearson correlation over all elements"""
    vx = output - torch.mean(output)
    vy = target - torch.mean(target)
    my_corr = torch.sum(vx * vy) / (torch.sqrt(torch.sum(vx ** 2)) * torch.sqrt(torch.sum(vy ** 2)))
    return my_corr ** 2


def get_true_val_set_r2(odenet, data_handler, method, batch_type):
    """The reference's `get_true_val_set_r2` (train_insilico.py:51-61): [r2, mse] of the noise-free validation pairs,
    every pair a one-row call over its own two times -- one per-sample launch.  Both figures stay on the device and the
    solver status is queued (engine.defer_status), so the function never waits for the GPU; an empty set gives NaN twice,
    as the reference's means over nothing do."""
    data_pw, t_pw, target_pw = data_handler.get_true_mu_set_pairwise(val_only=True, batch_type=batch_type)
    with torch.no_grad():
        if data_pw.shape[0] == 0:
            predictions_pw = torch.zeros(data_pw.shape, device=data_pw.device)
        else:
            y0, t, rtol, atol, method, options = _check_inputs(odenet, data_pw, t_pw, 1e-7, 1e-9, method, None)
            params, y2, t64, _B, _N, per_sample, t_is_f32, control = _prepare(odenet, y0, t, options)
            engine.check_pending_status()
            sol, status, _, _ = engine.solve_forward(engine.params_cached(*params), y2.detach().contiguous(), t64, method,
                                                     control, rtol, atol, per_sample, t_is_f32)
            engine.defer_status(status)
            predictions_pw = _out_shape(sol, y0, per_sample)[1]
        var_explained_pw = my_r_squared(predictions_pw, target_pw)
        true_val_mse = torch.mean((predictions_pw - target_pw) ** 2)
    return [var_explained_pw, true_val_mse]
