"""`phoenix_amd.training.validation` without a GPU: the solve it imports is replaced by a stub that runs the C oracle, and the
result is compared with a plain transcription of the reference's loop (train_insilico.py:77-106) on the same oracle.
Fixture: tests/golden/g9_data.csv, whose trajectories 0 and 3 miss their last time points."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CSV = os.path.join(GOLDEN, "g9_data.csv")


def _onet(oracle, net):
    import phoenix_amd
    ws, bs, wp, bp, wa, g = (x.detach().cpu().numpy() for x in phoenix_amd.odenet.params_of(net))
    return oracle.Net(ws, bs, wp, bp, wa, g.reshape(-1))


def _net(seed=5):
    import phoenix_amd
    torch.manual_seed(seed)
    net = phoenix_amd.ODENet("cpu", 10, neurons=6)
    with torch.no_grad():
        for prm in net.parameters():
            prm.add_(0.2 * torch.randn_like(prm))
    return net


def _oracle_odeint(oracle, net, y0, t, method):
    """odeint(net, y0 [rows, 1, N] or [rows, N], t [T]) -> [T, *y0.shape] on the oracle (one shared controller)"""
    sol = oracle.odeint(_onet(oracle, net), y0.numpy().astype(np.float32), t.numpy().astype(np.float64), method=method)
    return torch.from_numpy(np.asarray(sol, np.float32)).reshape((t.shape[0],) + tuple(y0.shape))


def _reference_loop(oracle, net, handler, method):
    """train_insilico.py:77-106, line by line, `odeint` being the oracle's"""
    data, t, target_full, n_val = handler.get_validation_set()
    predictions, targets = [], []
    for index, (time, batch_point, target_point) in enumerate(zip(t, data, target_full)):
        not_nan_idx = [i for i in range(len(time)) if not torch.isnan(time[i])]
        time = time[not_nan_idx]
        not_nan_idx.pop()
        batch_point = batch_point[not_nan_idx]
        target_point = target_point[not_nan_idx]
        predictions.append(_oracle_odeint(oracle, net, batch_point, time, method)[1])
        targets.append(target_point)
    predictions = torch.cat(predictions, dim=0)
    targets = torch.cat(targets, dim=0)
    return torch.mean((predictions - targets) ** 2), n_val, predictions, targets


def _handler(batch_type, seed):
    import phoenix_amd
    for s in range(seed, seed + 200):          # trajectory: a split whose validation set holds a trajectory with missing times
        np.random.seed(s)
        kw = {"batch_time": 3, "batch_time_frac": 0.5} if batch_type == "batch_time" else {}
        h = phoenix_amd.DataHandler.fromcsv(CSV, "cpu", 0.45 if batch_type == "trajectory" else 0.3, normalize=False,
                                            batch_type=batch_type, **kw)
        # (pairs / windows: the reference's own loop cannot run an item that lost a time point, its call has one time left)
        if bool(torch.isnan(h.val_t).any()) == (batch_type == "trajectory"):
            return h
    raise AssertionError("no split of the wanted kind")


@pytest.mark.parametrize("batch_type", ["trajectory", "single", "batch_time"])
@pytest.mark.parametrize("method", ["dopri5", "rk4"])
def test_validation_is_the_references_loop(oracle, monkeypatch, batch_type, method):
    from phoenix_amd import training
    net, h = _net(), _handler(batch_type, 40)
    if batch_type == "trajectory":
        nan_rows = torch.isnan(h.val_t).sum(1)
        assert nan_rows.max() > 0 and len(set(nan_rows.tolist())) > 1          # NaN filtering AND more than one group
    seen = []

    def stub_calls(func, y0s, t, rtol=1e-7, atol=1e-9, method=None, options=None):
        assert func is net and t.ndimension() == 2 and t.shape[0] == y0s.shape[0]
        seen.append(tuple(y0s.shape))
        return torch.stack([_oracle_odeint(oracle, net, y0s[k], t[k], method) for k in range(y0s.shape[0])])

    monkeypatch.setattr(training, "odeint_calls", stub_calls)
    loss, n_val = training.validation(net, h, method, False)
    pred, targ = training._validation_pairs(net, h, method)
    ref_loss, ref_n, ref_pred, ref_targ = _reference_loop(oracle, net, h, method)
    assert n_val == ref_n
    N = ref_pred.shape[-1]
    assert torch.equal(targ, ref_targ.reshape(-1, N))                # rows in the reference's order
    assert torch.equal(pred, ref_pred.reshape(-1, N))                # output 1 of every row, same oracle: bit for bit
    assert abs(loss.item() - ref_loss.item()) <= 1e-6 * abs(ref_loss.item())
    if batch_type == "trajectory":
        assert len({s[1] for s in seen}) > 1                         # one batched call per surviving row count


@pytest.mark.parametrize("case,batch_type", [("traj", "trajectory"), ("single", "single")])
@pytest.mark.parametrize("method", ["dopri5", "rk4"])
def test_oracle_meets_the_bar_of_the_validation_golden(oracle, monkeypatch, case, batch_type, method):
    """G19 (tests/golden/make_golden_validation.py: the reference's own `validation`) against `validation` on the C oracle,
    at the bar tests/test_gpu_parity.py holds `loss_data` of the G5 training step to -- the fixture is fit for the GPU test"""
    import phoenix_amd
    from conftest import load_golden, sub
    from phoenix_amd import training
    g = load_golden("g19_validation")
    p = sub(g, "p_")
    net = phoenix_amd.ODENet("cpu", 10, neurons=6)
    with torch.no_grad():
        net.net_sums.linear_out.weight.copy_(torch.from_numpy(p["Ws"]))
        net.net_sums.linear_out.bias.copy_(torch.from_numpy(p["bs"]))
        net.net_prods.linear_out.weight.copy_(torch.from_numpy(p["Wp"]))
        net.net_prods.linear_out.bias.copy_(torch.from_numpy(p["bp"]))
        net.net_alpha_combine.linear_out.weight.copy_(torch.from_numpy(p["Wa"]))
        net.gene_multipliers.copy_(torch.from_numpy(p["g"]).reshape(1, 10))
    np.random.seed(int(g[case + "/seed"]))
    h = phoenix_amd.DataHandler.fromcsv(CSV, "cpu", float(g[case + "/val_split"]), normalize=False, batch_type=batch_type)
    assert np.array_equal(h.val_t.numpy(), g[case + "/val_t"], equal_nan=True)          # the reference's split
    monkeypatch.setattr(training, "odeint_calls", lambda func, y0s, t, method=None: torch.stack(
        [_oracle_odeint(oracle, net, y0s[k], t[k], method) for k in range(y0s.shape[0])]))
    loss, n_val = training.validation(net, h, method, False)
    want = float(g["%s/%s/loss" % (case, method)])
    print(case, method, "loss", loss.item(), "golden", want, "rel", abs(loss.item() - want) / abs(want))
    assert n_val == int(g["%s/%s/n_val" % (case, method)])
    assert abs(loss.item() - want) < 1e-5 * abs(want)


@pytest.mark.parametrize("method", ["dopri5", "rk4", "euler"])
def test_output_one_needs_only_the_first_interval(oracle, method):
    """what `validation` relies on when it hands a call time[:2]: output 1 is the same with the whole grid"""
    net = _net(7)
    rs = np.random.RandomState(2)
    y0 = torch.from_numpy(rs.rand(5, 1, 10).astype(np.float32))
    for t in ([0.0, 1.0, 2.5, 3.0, 7.0], [4.0, 2.0, 1.5, 0.0], [1.0, 6.0, 6.5]):
        t = torch.tensor(t, dtype=torch.float64)
        full = _oracle_odeint(oracle, net, y0, t, method)
        two = _oracle_odeint(oracle, net, y0, t[:2], method)
        assert torch.equal(full[1], two[1]) and torch.equal(full[0], two[0])


def test_my_r_squared_and_names():
    import phoenix_amd
    x, y = torch.tensor([1.0, 2.0, 4.0, 3.0]), torch.tensor([2.0, 4.1, 8.0, 5.0])
    want = np.corrcoef(x.numpy(), y.numpy())[0, 1] ** 2
    assert abs(phoenix_amd.my_r_squared(x, y).item() - want) < 1e-6
    assert callable(phoenix_amd.validation) and callable(phoenix_amd.get_true_val_set_r2)
    empty = torch.zeros(0, 1, 10)
    assert torch.isnan(phoenix_amd.my_r_squared(empty, empty))
