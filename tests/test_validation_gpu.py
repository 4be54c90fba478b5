"""`phoenix_amd.validation` and `phoenix_amd.get_true_val_set_r2` on the MI355X against G19
(tests/golden/make_golden_validation.py: the reference's own two functions on tests/golden/g9_data.csv, whose validation
trajectories miss time points).  Run with `-m gpu`."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, sub
from test_gpu_parity import make_net

pytestmark = pytest.mark.gpu

CSV = os.path.join(GOLDEN, "g9_data.csv")
REL = 1e-5          # tests/test_gpu_parity.py, `loss_data` of the G5 training step: |got - want| < 1e-5 |want|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pa():
    import phoenix_amd
    return phoenix_amd


def _setup(pa, dev, g, case, batch_type):
    net = make_net(pa, dev, sub(g, "p_"))
    np.random.seed(int(g[case + "/seed"]))
    h = pa.DataHandler.fromcsv(CSV, dev, float(g[case + "/val_split"]), normalize=False, batch_type=batch_type)
    assert np.array_equal(h.val_t.cpu().numpy(), g[case + "/val_t"], equal_nan=True)        # the reference's split
    return net, h


@pytest.mark.parametrize("case,batch_type", [("traj", "trajectory"), ("single", "single")])
@pytest.mark.parametrize("method", ["dopri5", "rk4"])
def test_validation_against_the_reference(pa, dev, case, batch_type, method):
    g = load_golden("g19_validation")
    net, h = _setup(pa, dev, g, case, batch_type)
    if case == "traj":
        assert np.isnan(g[case + "/val_t"]).any()
    loss, n_val = pa.validation(net, h, method, False)
    want = float(g["%s/%s/loss" % (case, method)])
    print(case, method, "loss", loss.item(), "golden", want, "rel", abs(loss.item() - want) / abs(want))
    assert n_val == int(g["%s/%s/n_val" % (case, method)])
    assert abs(loss.item() - want) < REL * abs(want)


@pytest.mark.parametrize("case,batch_type", [("traj", "trajectory"), ("single", "single")])
@pytest.mark.parametrize("method", ["dopri5", "rk4"])
def test_true_val_set_r2_against_the_reference(pa, dev, case, batch_type, method):
    g = load_golden("g19_validation")
    net, h = _setup(pa, dev, g, case, batch_type)
    r2, mse = pa.get_true_val_set_r2(net, h, method, batch_type)
    assert r2.is_cuda and mse.is_cuda and r2.dim() == 0
    pa.check_pending_status(wait=True)
    for name, got in (("r2", r2.item()), ("mse", mse.item())):
        want = float(g["%s/%s/%s" % (case, method, name)])
        print(case, method, name, got, "golden", want, "rel", abs(got - want) / abs(want))
        assert abs(got - want) < REL * abs(want)
