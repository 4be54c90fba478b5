"""End-to-end pass through every row of the scope table on the device, the way the reference's `train_insilico.py` strings
them together (its driver itself is out of scope): simulate a data set with the Hill-kinetics simulator (f4) -> CSV wire
format -> DataHandler batches (f2) -> prior targets (f1) -> `training_step` with the fused solver, adjoint and prior
branch (a1-a13) under Adam -> validation solve (a14) -> checkpoint round trip -> influence scan (f3)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def test_simulate_train_validate_checkpoint_and_scan(tmp_path, monkeypatch):
    import phoenix_amd as pa
    from phoenix_amd.analysis import gene_influence_scores
    from phoenix_amd.prior import PriorMatrix, prior_targets
    from phoenix_amd.simulator import HillSystem, generate_dataset
    dev = torch.device("cuda:0")
    g = load_golden("g11_hill")
    system = HillSystem([str(x) for x in g["names"]], [str(x) for x in g["eqns"]], device=dev)
    N = system.N
    csv = str(tmp_path / "sim.csv")
    generate_dataset(system, 12, time_stamps=(0.0, 2.0, 3.0, 7.0, 9.0), expnoise=0.0, rng=np.random.default_rng(0), path=csv)
    np.random.seed(1)
    torch.manual_seed(1)
    handler = pa.DataHandler.fromcsv(csv, dev, 0.25, batch_type="trajectory", noise=0.0)
    assert handler.dim == N and handler.ntraj == 12
    net = pa.ODENet(dev, N, neurons=40)
    # a sparse sign prior (0.5 % dense) and its targets for a random prior batch (train_insilico.py:64-73, 207-211)
    rng = np.random.default_rng(2)
    nnz = int(0.005 * N * N)
    prior = PriorMatrix(rng.integers(0, N, nnz), rng.integers(0, N, nnz), rng.choice([-1.0, 1.0], nnz), N, dev)
    X = torch.rand(1500, 1, N, device=dev)
    prior_grad = prior_targets(X, prior)
    assert prior_grad.shape == X.shape and torch.isfinite(prior_grad).all()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    losses = []
    handler.reset_epoch()                                          # the driver's epoch loop (train_insilico.py:311)
    for step in range(25):
        if handler.epoch_done:
            handler.reset_epoch()
        loss_data, loss_prior = pa.training_step(net, handler, opt, "dopri5", 4, False, False, X, prior_grad, 0.99)
        losses.append((float(loss_data.detach()), float(loss_prior.detach())))
    assert all(np.isfinite(l).all() for l in losses)
    first, last = np.mean([l[0] for l in losses[:5]]), np.mean([l[0] for l in losses[-5:]])
    assert last < 0.9 * first, (first, last)                      # the data loss goes down
    # validation: one shared-control solve over a whole trajectory's time grid (train_insilico.py:77-106)
    data, t = handler.data_pt[0], handler.time_pt[0]
    with torch.no_grad():
        pred = pa.odeint_adjoint(net, data[0].reshape(1, 1, N), t, method="dopri5")
    assert pred.shape == (len(t), 1, 1, N) and torch.isfinite(pred).all()
    # checkpoint round trip: same predictions from a reloaded network (save() inserts its suffixes at the FIRST '.' of
    # the path, as the reference does: a relative name keeps a dot in the temporary directory's path out of it)
    monkeypatch.chdir(tmp_path)
    fp = "ckpt.pt"
    net.save(fp)
    net2 = pa.ODENet(dev, N, neurons=40)
    net2.load(fp)
    with torch.no_grad():
        pred2 = pa.odeint_adjoint(net2, data[0].reshape(1, 1, N), t, method="dopri5")
    assert torch.equal(pred, pred2)
    # influence scan of a few genes with the trained network
    scores = gene_influence_scores(net, N, "dopri5", n_random_inputs_per_gene=20, device=dev, genes=[0, 17, 349])
    assert scores.shape == (3,) and np.all(np.isfinite(scores)) and np.all(scores >= 0)
    assert os.path.exists(csv)
