#!/usr/bin/env python3
"""Generate the golden fixtures that pin the oracle (and, through it, the HIP engine).

Runs ONLY in the build container, where the reference is mounted read-only at /root/reference:
it imports the reference's own `ODENet`, `odeint`, `odeint_adjoint` and (by AST extraction, the
module itself is a script) `training_step`, runs them on small seeded inputs and stores
inputs + outputs as .npz files next to this script.  The fixtures are data only; no reference
source travels.  Re-run with:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens.py

Goldens:
  G1 rhs            ODENet.forward / prior_only_forward                    (odenet.py:85-98)
  G2 rhs_vjp        torch.autograd.grad(f, (y, *params), cot)              (adjoint.py:116-119)
  G3 fixed          odeint / odeint_adjoint with euler, midpoint, rk4      (fixed_grid.py, solvers.py)
  G4 dopri5         odeint / odeint_adjoint, per-sample, batched, fp64 t, decreasing t
  G5 training_step  one full reference training_step + Adam update         (train_insilico.py:124-140)
  G6 controller     _select_initial_step pieces, error ratio, step size, interpolation, norms
  G7 realdata       first pairs of shipped yeast / breast CSVs with a seeded H=8 net
  G9 datahandler    readcsv + DataHandler split / batches / validation sets, numpy stream seeded (datahandler.py, csvreader.py)
  G10 analysis      gene-influence scoring loop (find_gene_influences.py:64-77) and calculate_trajectory (datahandler.py:310-340)
  G12 spread        the reference's OWN dopri5 gradients at rtol * {0.85 ... 1.15} and an fp64 tight-tolerance truth (G4 inputs)
  G11 hill          rate expressions of the 350-gene ground-truth network: rates and LSODA trajectories (GraphGRN_core.R:425-486)
  G13 hill690       the same for the 690-gene network (ode_system_functions_690.csv)
  G8 prior          read_prior_matrix (dense + triplet formats) and prior_grad = X @ P   (train_insilico.py:64-73,207-211)
  G14 breast11165   the reference at FULL size on the shipped 11 165-gene test sample (7 pairs, H = 40, config_breast.cfg):
                    its own ODENet (sparse_ init), the training loop's per-sample odeint_adjoint calls, loss_data, backward
  G15 yeast3551     the same on the shipped 3 551-gene yeast sample (23 pairs, dt = 5, H = 120, config_yeast.cfg)
  G25 dopri5_truth  (make_golden_truth.py) an fp64 tight-tolerance truth at the shapes of every dopri5 kernel family -- fwd3 /
                    adj3 past 32 gene blocks, fwd3c / adj3c at 2 ... 6 hidden chunks -- with unit and training-scale cotangents,
                    and the reference's own float32 errors against it at rtol * {0.85 ... 1.15}, batched and per sample
  G26 fixed_truth   (make_golden_fixed_truth.py) the reference's odeint_adjoint with euler / midpoint / rk4 in float64, with and
                    without options["step_size"] and with a backward step of its own: the anchor of the float64 arbiter
                    (tests/g26.py) that the fixed-grid kernels are held to at every launch geometry
"""
import ast
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference/ode_net/code"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from odenet import ODENet  # noqa: E402  (reference)
from torchdiffeq import odeint, odeint_adjoint  # noqa: E402  (reference, vendored 0.1.1)
from torchdiffeq._impl import misc as ref_misc  # noqa: E402
from torchdiffeq._impl import interp as ref_interp  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(1)


def make_net(N, H, seed, dense_std=None, neg_g_frac=0.0):
    """Reference ODENet; `dense_std` overwrites the 95%-sparse init with a trained-like dense one
    (Adam densifies the factors)."""
    torch.manual_seed(seed)
    net = ODENet("cpu", N, explicit_time=False, neurons=H).float()
    if dense_std is not None:
        with torch.no_grad():
            for lin in (net.net_sums.linear_out, net.net_prods.linear_out, net.net_alpha_combine.linear_out):
                lin.weight.normal_(0.0, dense_std)
            net.net_sums.linear_out.bias.uniform_(-0.2, 0.2)
            net.net_prods.linear_out.bias.uniform_(-0.2, 0.2)
    if neg_g_frac > 0:
        with torch.no_grad():
            m = torch.rand(1, N) < neg_g_frac
            net.gene_multipliers[m] = -net.gene_multipliers[m]  # relu() clamps these genes to 0
    return net


def params_np(net):
    return {
        "Ws": net.net_sums.linear_out.weight.detach().numpy().copy(),
        "bs": net.net_sums.linear_out.bias.detach().numpy().copy(),
        "Wp": net.net_prods.linear_out.weight.detach().numpy().copy(),
        "bp": net.net_prods.linear_out.bias.detach().numpy().copy(),
        "Wa": net.net_alpha_combine.linear_out.weight.detach().numpy().copy(),
        "g": net.gene_multipliers.detach().numpy().reshape(-1).copy(),
    }


def grads_np(net, prefix="grad_"):
    def g(p):
        return (torch.zeros_like(p) if p.grad is None else p.grad).detach().numpy().copy()

    return {
        prefix + "Ws": g(net.net_sums.linear_out.weight),
        prefix + "bs": g(net.net_sums.linear_out.bias),
        prefix + "Wp": g(net.net_prods.linear_out.weight),
        prefix + "bp": g(net.net_prods.linear_out.bias),
        prefix + "Wa": g(net.net_alpha_combine.linear_out.weight),
        prefix + "g": g(net.gene_multipliers).reshape(-1),
    }


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print("wrote %-28s %6.1f KB  keys=%d" % (name + ".npz", os.path.getsize(path) / 1024, len(arrs)))


def pfx(d, p):
    return {p + k: v for k, v in d.items()}


# ---------------------------------------------------------------- G1 / G2
def g1_g2():
    out = {}
    cases = [("sparse", 48, 8, None, 0.0), ("dense", 48, 8, 0.15, 0.25), ("odd", 37, 5, 0.2, 0.2)]
    for name, N, H, std, neg in cases:
        net = make_net(N, H, seed=11, dense_std=std, neg_g_frac=neg)
        torch.manual_seed(5)
        y = torch.rand(6, 1, N) * 7 - 3  # [-3, 4]
        y[0, 0, :4] = torch.tensor([0.5, 0.5 + 1e-7, 50.0, -50.0])  # kink + large magnitudes
        y1 = torch.rand(1, N) * 1.2 - 0.1
        f = net(torch.tensor(0.0), y).detach()
        fp = net.prior_only_forward(torch.tensor(0.0), y).detach()
        f1 = net(torch.tensor(0.0), y1).detach()
        # VJP
        yv = y.clone().requires_grad_(True)
        cot = torch.randn(6, 1, N)
        fv = net(torch.tensor(0.0), yv)
        gr = torch.autograd.grad(fv, (yv,) + tuple(net.parameters()), cot)
        names = [n for n, _ in net.named_parameters()]
        gmap = dict(zip(names, gr[1:]))
        # prior_only VJP
        yv2 = y.clone().requires_grad_(True)
        fv2 = net.prior_only_forward(torch.tensor(0.0), yv2)
        gr2 = torch.autograd.grad(fv2, (yv2,) + tuple(net.parameters()), cot, allow_unused=True)
        gmap2 = dict(zip(names, gr2[1:]))

        def gm(m, N=N):
            z = lambda k, shape: (m[k] if m[k] is not None else torch.zeros(shape)).numpy()
            H_ = m["net_sums.linear_out.bias"].shape[0]
            return {
                "Ws": z("net_sums.linear_out.weight", (H_, N)), "bs": z("net_sums.linear_out.bias", (H_,)),
                "Wp": z("net_prods.linear_out.weight", (H_, N)), "bp": z("net_prods.linear_out.bias", (H_,)),
                "Wa": z("net_alpha_combine.linear_out.weight", (N, 2 * H_)),
                "g": z("gene_multipliers", (1, N)).reshape(-1),
            }

        d = dict(y=y.numpy(), f=f.numpy(), f_prior=fp.numpy(), y1=y1.numpy(), f1=f1.numpy(), cot=cot.numpy(),
                 vjp_y=gr[0].numpy(), vjp_y_prior=gr2[0].numpy())
        d.update(pfx(params_np(net), "p_"))
        d.update(pfx(gm(gmap), "vjp_"))
        d.update(pfx(gm(gmap2), "vjpprior_"))
        out.update(pfx(d, name + "/"))
    save("g1_g2_rhs", **out)


# ---------------------------------------------------------------- G3 / G4 helpers
def run_adjoint(net, y0, t, method, G):
    """loss = sum(G * odeint_adjoint(...)); returns sol, y0.grad, param grads."""
    for p in net.parameters():
        p.grad = None
    y0 = y0.clone().requires_grad_(True)
    sol = odeint_adjoint(net, y0, t, method=method)
    (sol * G).sum().backward()
    return sol.detach().numpy(), y0.grad.numpy().copy(), grads_np(net)


def g3_fixed():
    out = {}
    N, H = 40, 6
    net = make_net(N, H, seed=3, dense_std=0.12, neg_g_frac=0.15)
    out.update(pfx(params_np(net), "p_"))
    torch.manual_seed(7)
    y0_single = torch.rand(1, N)
    y0_batch = torch.rand(5, 1, N) * 1.5 - 0.25
    t2 = torch.tensor([0.0, 2.0])
    t5 = torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0])  # simulator time stamps
    t5_64 = t5.double() * 0.1 + 0.013
    t_dec = torch.tensor([1.0, 0.6, 0.1])
    out.update(y0_single=y0_single.numpy(), y0_batch=y0_batch.numpy(), t2=t2.numpy(), t5=t5.numpy(),
               t5_64=t5_64.numpy(), t_dec=t_dec.numpy())
    for method in ("euler", "midpoint", "rk4"):
        for tname, t in (("t2", t2), ("t5", t5), ("t5_64", t5_64), ("t_dec", t_dec)):
            for yname, y0 in (("single", y0_single), ("batch", y0_batch)):
                with torch.no_grad():
                    sol = odeint(net, y0, t, method=method)
                key = "%s/%s/%s/" % (method, tname, yname)
                out[key + "sol"] = sol.numpy()
                if tname in ("t2", "t5", "t_dec"):
                    torch.manual_seed(13)
                    G = torch.randn(sol.shape)
                    s2, gy0, gp = run_adjoint(net, y0, t, method, G)
                    assert np.array_equal(s2, sol.numpy())
                    out[key + "G"] = G.numpy()
                    out[key + "grad_y0"] = gy0
                    out.update(pfx(gp, key))
    save("g3_fixed", **out)


def g4_dopri5():
    out = {}
    N, H = 32, 6
    net = make_net(N, H, seed=21, dense_std=0.2, neg_g_frac=0.1)
    out.update(pfx(params_np(net), "p_"))
    torch.manual_seed(9)
    y0_single = torch.rand(1, N) * 1.4 - 0.2
    y0_batch = torch.rand(4, 1, N) * 1.4 - 0.2
    t2 = torch.tensor([0.0, 1.5])
    t4 = torch.tensor([0.0, 0.5, 1.25, 3.0])
    t10_64 = torch.arange(0, 1, 0.1, dtype=torch.float64)
    t_dec = torch.tensor([2.0, 1.0, 0.25])
    out.update(y0_single=y0_single.numpy(), y0_batch=y0_batch.numpy(), t2=t2.numpy(), t4=t4.numpy(),
               t10_64=t10_64.numpy(), t_dec=t_dec.numpy())
    for tname, t in (("t2", t2), ("t4", t4), ("t10_64", t10_64), ("t_dec", t_dec)):
        for yname, y0 in (("single", y0_single), ("batch", y0_batch)):
            with torch.no_grad():
                sol = odeint(net, y0, t)  # default method = dopri5, rtol 1e-7, atol 1e-9
            key = "%s/%s/" % (tname, yname)
            out[key + "sol"] = sol.numpy()
            if tname != "t10_64":
                torch.manual_seed(17)
                G = torch.randn(sol.shape)
                s2, gy0, gp = run_adjoint(net, y0, t, "dopri5", G)
                out[key + "G"] = G.numpy()
                out[key + "grad_y0"] = gy0
                out.update(pfx(gp, key))
            # fp64 tight-tolerance "truth" of the same ODE
            net64 = make_net(N, H, seed=21, dense_std=0.2, neg_g_frac=0.1).double()
            with torch.no_grad():
                truth = odeint(net64, y0.double(), t.double(), rtol=1e-12, atol=1e-14)
            out[key + "truth64"] = truth.numpy()
    # per-sample loop (the training-loop semantics, train_insilico.py:128-130)
    tb = torch.tensor([[0.0, 0.7], [0.3, 1.9], [1.0, 1.2], [0.0, 2.5]])
    preds = []
    for p in net.parameters():
        p.grad = None
    y0b = y0_batch.clone().requires_grad_(True)
    for time, yp in zip(tb, y0b):
        preds.append(odeint_adjoint(net, yp, time)[1])
    pred = torch.stack(preds)
    torch.manual_seed(19)
    G = torch.randn(pred.shape)
    (pred * G).sum().backward()
    out.update({"loop/t": tb.numpy(), "loop/pred": pred.detach().numpy(), "loop/G": G.numpy(),
                "loop/grad_y0": y0b.grad.numpy().copy()})
    out.update(pfx(grads_np(net), "loop/"))
    save("g4_dopri5", **out)


# ---------------------------------------------------------------- G5
def load_reference_training_step():
    """The reference's train_insilico.py is a script (argparse at import); lift its
    `training_step` function object out by AST and bind it to the reference's odeint_adjoint,
    exactly as the script does (`from torchdiffeq import odeint_adjoint as odeint`, :15-18)."""
    src = open(os.path.join(REF, "train_insilico.py")).read()
    tree = ast.parse(src)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "training_step"]
    assert len(fn) == 1
    mod = ast.Module(body=fn, type_ignores=[])
    ns = {"torch": torch, "odeint": odeint_adjoint}
    exec(compile(mod, "<reference train_insilico.py:training_step>", "exec"), ns)
    return ns["training_step"]


class FakeHandler:
    """Minimal stand-in for DataHandler.get_batch (datahandler.py:87-93): fixed tensors."""
    device = "cpu"

    def __init__(self, batch, t, target):
        self.b = (batch, t, target)

    def get_batch(self, bs):
        return self.b


def g5_training_step():
    training_step = load_reference_training_step()
    out = {}
    N, H, B, K = 36, 6, 4, 32
    for method in ("dopri5", "rk4"):
        for lam in (0.99, 1.0):
            net = make_net(N, H, seed=33, dense_std=0.15, neg_g_frac=0.1)
            torch.manual_seed(41)
            batch = torch.rand(B, 1, N)
            t = torch.tensor([[0.0, 2.0], [2.0, 3.0], [3.0, 7.0], [7.0, 9.0]]) * 0.25
            target = batch + 0.1 * torch.randn(B, 1, N)
            X = torch.rand(K, 1, N) - 0.5
            Pm = (torch.rand(N, N) < 0.03).float() * torch.sign(torch.randn(N, N))
            prior_grad = torch.matmul(X, Pm)  # train_insilico.py:209-210
            lr = 1e-3
            opt = torch.optim.Adam([  # train_insilico.py:244-253
                {"params": net.net_sums.linear_out.weight}, {"params": net.net_sums.linear_out.bias},
                {"params": net.net_prods.linear_out.weight}, {"params": net.net_prods.linear_out.bias},
                {"params": net.net_alpha_combine.linear_out.weight},
                {"params": net.gene_multipliers, "lr": 5 * lr}], lr=lr, weight_decay=0)
            key = "%s/lam%g/" % (method, lam)
            out.update(pfx(params_np(net), key + "p_"))
            # predictions (the function does not return them): same loop, no grad
            with torch.no_grad():
                pred = torch.stack([odeint(net, bp, tt, method=method)[1] for tt, bp in zip(t, batch)])
            loss_data, loss_prior = training_step(net, FakeHandler(batch, t, target), opt, method, B, False,
                                                  False, X, prior_grad, lam)
            out.update({key + "batch": batch.numpy(), key + "t": t.numpy(), key + "target": target.numpy(),
                        key + "X": X.numpy(), key + "prior_grad": prior_grad.numpy(), key + "pred": pred.numpy(),
                        key + "loss_data": loss_data.item(), key + "loss_prior": loss_prior.item(),
                        key + "lr": lr})
            out.update(pfx(grads_np(net), key))
            out.update(pfx(params_np(net), key + "after_"))
    save("g5_training_step", **out)


# ---------------------------------------------------------------- G6
def g6_controller():
    out = {}
    torch.manual_seed(2)
    n = 50
    x = torch.randn(n)
    out["norm/x"] = x.numpy()
    out["norm/rms"] = ref_misc._rms_norm(x).item()
    shapes = [torch.Size(()), torch.Size((1, 12)), torch.Size((1, 12)), torch.Size((25,))]
    out["norm/blocks"] = np.array([1, 12, 12, 25])
    out["norm/mixed"] = float(ref_misc._mixed_linf_rms_norm(shapes)(x))
    # _optimal_step_size
    ers = [0.0, 1e-4, 0.3, 0.999, 1.0, 1.7, 50.0, 1e6]
    res = []
    for er in ers:
        r = ref_misc._optimal_step_size(torch.tensor(0.125, dtype=torch.float64), torch.tensor(er, dtype=torch.float32),
                                        torch.tensor(0.9, dtype=torch.float64), torch.tensor(10.0, dtype=torch.float64),
                                        torch.tensor(0.2, dtype=torch.float64), 5)
        res.append(float(r))
    out["step/error_ratio"] = np.array(ers, np.float32)
    out["step/dt_next"] = np.array(res, np.float64)
    # interpolation
    y0, y1, ym, f0, f1 = [torch.randn(n) for _ in range(5)]
    dt = torch.tensor(0.37)
    coef = ref_interp._interp_fit(y0, y1, ym, f0, f1, dt)
    out.update({"interp/y0": y0.numpy(), "interp/y1": y1.numpy(), "interp/ym": ym.numpy(), "interp/f0": f0.numpy(),
                "interp/f1": f1.numpy(), "interp/dt": dt.item(), "interp/coef": torch.stack(coef).numpy()})
    t0, t1 = torch.tensor(1.0, dtype=torch.float64), torch.tensor(1.37, dtype=torch.float64)
    ts = [1.0, 1.1, 1.2345, 1.37]
    out["interp/ts"] = np.array(ts)
    out["interp/vals"] = np.stack([ref_interp._interp_evaluate(coef, t0, t1, torch.tensor(tt, dtype=torch.float64)).numpy()
                                   for tt in ts])
    # _select_initial_step + error ratio on a real net
    N, H = 24, 4
    net = make_net(N, H, seed=8, dense_std=0.2)
    out.update(pfx(params_np(net), "init/p_"))
    yy = torch.rand(1, N)
    rtol = torch.tensor(1e-7, dtype=torch.float64)
    atol = torch.tensor(1e-9, dtype=torch.float64)
    with torch.no_grad():
        func = lambda t, y: net(t.type_as(y), y)
        h = ref_misc._select_initial_step(func, torch.tensor(0.0, dtype=torch.float64), yy, 4, rtol, atol,
                                          ref_misc._rms_norm)
    out["init/y0"] = yy.numpy()
    out["init/h"] = float(h)
    e, a, b = torch.randn(n) * 1e-7, torch.randn(n), torch.randn(n)
    out.update({"ratio/err": e.numpy(), "ratio/y0": a.numpy(), "ratio/y1": b.numpy(),
                "ratio/value": float(ref_misc._compute_error_ratio(e, rtol, atol, a, b, ref_misc._rms_norm))})
    save("g6_controller", **out)


# ---------------------------------------------------------------- G7
def read_ref_csv(path, n_pairs):
    """csvreader.readcsv format (csvreader.py:13-56): row0 = dim,ntraj; per trajectory `dim`
    expression rows then one time row."""
    import csv
    with open(path) as fh:
        rows = list(csv.reader(fh))
    dim, ntraj = int(float(rows[0][0])), int(float(rows[0][1]))
    expr = np.array([[float(v) if v != "" else np.nan for v in r] for r in rows[1:1 + dim]], np.float32)  # [dim, T]
    tt = np.array([float(v) if v != "" else np.nan for v in rows[1 + dim]], np.float32)
    return expr.T[: n_pairs + 1].copy(), tt[: n_pairs + 1].copy(), dim


def g7_realdata():
    out = {}
    files = {
        "yeast": "/root/reference/pramila_yeast_data/clean_data/pramila_500genes_1sample_24T.csv",
        "breast": "/root/reference/breast_cancer_data/clean_data/desmedt_500genes_1sample_178T.csv",
    }
    for name, path in files.items():
        Y, tt, dim = read_ref_csv(path, 2)
        NG = 64  # first 64 genes keep the fixture small
        Y = Y[:, :NG]
        net = make_net(NG, 8, seed=77, dense_std=0.1)
        key = name + "/"
        out.update(pfx(params_np(net), key + "p_"))
        out[key + "Y"] = Y
        out[key + "t"] = tt
        for i in range(2):
            y0 = torch.from_numpy(Y[i:i + 1])
            t = torch.from_numpy(tt[i:i + 2])
            torch.manual_seed(23 + i)
            G = torch.randn(2, 1, NG)
            sol, gy0, gp = run_adjoint(net, y0, t, "dopri5", G)
            out[key + "pair%d/sol" % i] = sol
            out[key + "pair%d/G" % i] = G.numpy()
            out[key + "pair%d/grad_y0" % i] = gy0
            out.update(pfx(gp, key + "pair%d/" % i))
    save("g7_realdata", **out)


# ---------------------------------------------------------------- G8 (row f1: prior targets)
def load_reference_function(name):
    src = open(os.path.join(REF, "train_insilico.py")).read()
    tree = ast.parse(src)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fn) == 1
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "<reference train_insilico.py:%s>" % name, "exec"), ns)
    return ns[name]


def g8_prior():
    import tempfile
    read_prior_matrix = load_reference_function("read_prior_matrix")   # train_insilico.py:64-73
    out = {}
    # (a) the shipped dense in-silico prior, 350 x 350, and the prior targets of a seeded batch
    path = "/root/reference/ground_truth_simulator/clean_data/edge_prior_matrix_G350_noise_0.0.csv"
    P = read_prior_matrix(path, sparse=False, num_genes=350)
    r, c = np.nonzero(P.numpy())
    torch.manual_seed(4)
    X = torch.rand(16, 1, 350) - 0.5
    out.update({"g350/rows": r, "g350/cols": c, "g350/vals": P.numpy()[r, c], "g350/X": X.numpy(),
                "g350/prior_grad": torch.matmul(X, P).numpy(), "g350/csv_rows": np.genfromtxt(path, delimiter=",")[:3]})
    # (b) triplet format (1-based i,j,v; duplicates are summed by sparse_coo_tensor.to_dense())
    rs = np.random.RandomState(6)
    n = 40
    trip = np.stack([rs.randint(1, n + 1, 90), rs.randint(1, n + 1, 90), rs.choice([-1.0, 0.5, 1.0], 90)], 1)
    trip[5] = trip[4]   # a duplicate coordinate
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as fh:
        for a, b, v in trip:
            fh.write("%d,%d,%g\n" % (a, b, v))
        tpath = fh.name
    Ps = read_prior_matrix(tpath, sparse=True, num_genes=n)
    os.unlink(tpath)
    Xs = torch.rand(8, 1, n) - 0.5
    out.update({"trip/triplets": trip, "trip/dense": Ps.numpy(), "trip/X": Xs.numpy(),
                "trip/prior_grad": torch.matmul(Xs, Ps).numpy(),
                "trip/prior_grad_abs": torch.matmul(Xs, torch.abs(Ps)).numpy()})
    save("g8_prior", **out)


# ---------------------------------------------------------------- G9 (row f2: csv format + DataHandler batching)
def g9_datahandler():
    """Reference DataHandler (datahandler.py) over a small synthetic CSV in the shipped wire format, with the global
    numpy stream seeded: noise draws, train/validation split and every batch of one epoch are recorded."""
    import contextlib
    import io
    from datahandler import DataHandler as RefDataHandler     # reference (needs matplotlib + figure_saver only at import)
    csv_path = os.path.join(OUT, "g9_data.csv")
    rs = np.random.RandomState(9)
    dim, ntraj, L = 10, 7, 6
    with open(csv_path, "w") as fh:
        fh.write("%d,%d\n" % (dim, ntraj))
        for tr in range(ntraj):
            nvalid = L if tr % 3 else L - 1 - (tr % 2)          # some trajectories miss their last time points
            for d in range(dim):
                vals = rs.rand(L)
                fh.write(",".join(("%.6f" % v) if i < nvalid else "" for i, v in enumerate(vals)) + "\n")
            times = np.cumsum(rs.randint(1, 4, L)).astype(float)
            fh.write(",".join(("%g" % v) if i < nvalid else "" for i, v in enumerate(times)) + "\n")
    out = {}

    def rec(key, b, t, y):
        out[key + "/batch"], out[key + "/t"], out[key + "/target"] = b.numpy(), t.numpy(), y.numpy()

    def epoch(h, key, bs):
        h.reset_epoch()
        k = 0
        while not h.epoch_done:
            rec("%s/b%d" % (key, k), *h.get_batch(bs))
            k += 1
        out[key + "/n_batches"] = k

    with contextlib.redirect_stdout(io.StringIO()):
        np.random.seed(101)
        h = RefDataHandler.fromcsv(csv_path, "cpu", 0.2, normalize=False, batch_type="single", noise=0.05,
                                   scale_expression=2.0)
        vd, vt, vy, nv = h.get_validation_set()
        rec("A/val", vd, vt, vy)
        out["A/n_val"] = nv
        out["A/data_np0"] = h.data_np[0]
        out["A/data_np0_0noise"] = h.data_np_0noise[0]
        epoch(h, "A", 5)
        rec("A/mu_val", *h.get_true_mu_set_pairwise(val_only=True, batch_type="single"))
        rec("A/mu_all", *h.get_true_mu_set_pairwise(val_only=False, batch_type="single"))

        np.random.seed(202)
        h = RefDataHandler.fromcsv(csv_path, "cpu", 0.3, normalize=True, batch_type="trajectory", noise=0.0)
        vd, vt, vy, nv = h.get_validation_set()
        rec("B/val", vd, vt, vy)
        out["B/n_val"] = nv
        out["B/val_set_indx"] = np.asarray(h.val_set_indx)
        epoch(h, "B", 1)
        rec("B/mu_val", *h.get_true_mu_set_pairwise(val_only=True, batch_type="trajectory"))
        rec("B/init_val", *h.get_true_mu_set_init_val_based())
        out["B/times"] = h.get_times().numpy()

        np.random.seed(303)
        h = RefDataHandler.fromcsv(csv_path, "cpu", 0.2, batch_type="batch_time", batch_time=3, batch_time_frac=0.5)
        vd, vt, vy, nv = h.get_validation_set()
        rec("C/val", vd, vt, vy)
        out["C/n_val"] = nv
        epoch(h, "C", 4)
    save("g9_datahandler", **out)


# ---------------------------------------------------------------- G10 (row f3: batched analysis callers)
def g10_analysis():
    """(a) the scoring loop of find_gene_influences.py:64-77 (a script, so restated here call for call around the
    reference's own odeint / ODENet) with the random draws recorded; (b) DataHandler.calculate_trajectory."""
    import contextlib
    import io
    from datahandler import DataHandler as RefDataHandler
    out = {}
    N, H, S = 24, 6, 8
    net = make_net(N, H, seed=31, dense_std=0.15, neg_g_frac=0.1)
    out.update(pfx(params_np(net), "infl/p_"))
    torch.manual_seed(12)
    time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))
    inits, perts, scores = [], [], []
    with torch.no_grad():
        for this_gene in range(N):
            this_init = 1 * (torch.rand(S, 1, N) - 0.5)
            inits.append(this_init.numpy().copy())
            unpert_out = odeint_adjoint(net, this_init, time_pts_to_project, method="dopri5")
            this_pert_col = 1 * (torch.rand(S) - 0.5)
            perts.append(this_pert_col.numpy().copy())
            this_init[:, 0, this_gene] = this_pert_col
            pert_out = odeint_adjoint(net, this_init, time_pts_to_project, method="dopri5")
            all_other_genes = [idx for idx in range(N) if idx != this_gene]
            scores.append(torch.mean(abs(unpert_out[1:, :, :, all_other_genes] - pert_out[1:, :, :, all_other_genes])).item())
    out.update({"infl/inits": np.stack(inits), "infl/perts": np.stack(perts), "infl/scores": np.array(scores)})

    csv_path = os.path.join(OUT, "g9_data.csv")
    net2 = make_net(10, 6, seed=5, dense_std=0.2)
    out.update(pfx(params_np(net2), "traj/p_"))
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        np.random.seed(404)
        h = RefDataHandler.fromcsv(csv_path, "cpu", 0.3, batch_type="trajectory", noise=0.0)
        trajs, samples, grid = h.calculate_trajectory(net2, "dopri5", num_val_trajs=2)
    out.update({"traj/trajectories": np.stack([x.numpy() for x in trajs]), "traj/samples": np.asarray(samples),
                "traj/grid": grid})
    save("g10_analysis", **out)


# ---------------------------------------------------------------- G11 (row f4: Hill-kinetics simulator)
def g11_hill():
    """The shipped 350-gene rate expressions (reference DATA: ground_truth_simulator/clean_data/
    ode_system_functions_350.csv, emitted by GraphGRN_core.R:425-486) go into the fixture as input arrays (node names,
    expression strings); their rates on random states are Python's own fp64 evaluation of the strings with fAct as defined in
    GraphGRN_core.R:431-436, trajectories are scipy LSODA at rtol 1e-10 (the reference uses deSolve's lsoda).
    R cannot run here, so the reference's own simulated data set cannot be regenerated: parity of f4 is pinned
    against the expression files only."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from oracle import hill_oracle
    from phoenix_amd.simulator import read_ode_system
    names, exprs = read_ode_system("/root/reference/ground_truth_simulator/clean_data/ode_system_functions_350.csv")
    rs = np.random.RandomState(11)
    X = rs.rand(16, len(names))
    X[0, :5] = 0.0                                   # fAct(0) = 0 branch
    rates = hill_oracle.rhs(names, exprs, X)
    times = np.array([0.0, 2.0, 3.0, 7.0, 9.0])      # example_creator_for_chalmers_codebase_0noise.R:134
    x0 = np.clip(rs.beta(2, 2, size=(3, len(names))) + rs.uniform(-0.25, 0.25, size=(1, len(names))), 0, 1)
    traj = np.stack([hill_oracle.simulate(names, exprs, x0[i], times) for i in range(3)], 1)   # [T, 3, N]
    save("g11_hill", names=np.array(names), eqns=np.array(exprs), X=X, rates=rates, times=times, x0=x0, traj=traj)


def g16_edges():
    """The shipped edge tables of the two in-silico networks (reference DATA: ground_truth_simulator/clean_data/
    edge_properties_G350.csv / _G690.csv -- from, to, weight, activation, EC50, n exactly as R printed them) as text arrays:
    the inputs from which GraphGRN_core.R:163-190,221-236 builds the rate-expression strings of G11 / G13.  Pins the
    equation builder of phoenix_amd/simulator.py (rate_expression) text for text at 350 genes; the shipped 690-gene table
    comes from another draw of the random EC50 / n than the shipped 690-gene expressions (every value differs), so there
    only the structure (every regulator is an edge, negated exactly where activation is FALSE) can be held."""
    import csv
    out = {}
    for tag in ("350", "690"):
        rows = list(csv.DictReader(open("/root/reference/ground_truth_simulator/clean_data/edge_properties_G%s.csv" % tag)))
        for k in ("from", "to", "weight", "activation", "EC50", "n"):
            out["e%s_%s" % (tag, k)] = np.array([r[k] for r in rows])
    save("g16_edges", **out)


def g13_hill690():
    """G11 for the second shipped network: ground_truth_simulator/clean_data/ode_system_functions_690.csv (690 nodes).
    Same recipe -- expression strings as input arrays, Python fp64 rates on random states, scipy LSODA trajectories."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from oracle import hill_oracle
    from phoenix_amd.simulator import read_ode_system
    names, exprs = read_ode_system("/root/reference/ground_truth_simulator/clean_data/ode_system_functions_690.csv")
    rs = np.random.RandomState(13)
    X = rs.rand(8, len(names))
    X[0, :5] = 0.0
    rates = hill_oracle.rhs(names, exprs, X)
    times = np.array([0.0, 2.0, 3.0, 7.0, 9.0])
    x0 = np.clip(rs.beta(2, 2, size=(2, len(names))) + rs.uniform(-0.25, 0.25, size=(1, len(names))), 0, 1)
    traj = np.stack([hill_oracle.simulate(names, exprs, x0[i], times) for i in range(2)], 1)   # [T, 2, N]
    save("g13_hill690", names=np.array(names), eqns=np.array(exprs), X=X, rates=rates, times=times, x0=x0, traj=traj)


# ---------------------------------------------------------------- G12 (spread of the reference's own gradients)
def g12_spread():
    """rtol = 1e-7 is below fp32 epsilon: accept/reject decisions of the adaptive solver are rounding noise, so the
    reference's own fp32 gradient moves when rtol is jittered.  This captures how far: its gradients at
    rtol * {0.85 ... 1.15} (seven values) and the fp64 tight-tolerance gradient of the same problem, for every G4 case that has
    gradients.  tests assert that the engine (and the oracle) are no further from the truth than the reference is."""
    g4 = np.load(os.path.join(OUT, "g4_dopri5.npz"))
    out = {}
    N, H = 32, 6
    net = make_net(N, H, seed=21, dense_std=0.2, neg_g_frac=0.1)
    net64 = make_net(N, H, seed=21, dense_std=0.2, neg_g_frac=0.1).double()

    def grads_of_run(nn, y0, t, G, rtol, atol):
        for p in nn.parameters():
            p.grad = None
        y = y0.clone().requires_grad_(True)
        sol = odeint_adjoint(nn, y, t, rtol=rtol, atol=atol)
        (sol * G).sum().backward()
        d = {"grad_y0": y.grad.numpy().copy()}
        d.update(grads_np(nn))
        return d

    for tname in ("t2", "t4", "t_dec"):
        for yname in ("single", "batch"):
            key = "%s/%s/" % (tname, yname)
            y0 = torch.from_numpy(g4["y0_" + yname])
            t = torch.from_numpy(g4[tname])
            G = torch.from_numpy(g4[key + "G"])
            truth = grads_of_run(net64, y0.double(), t.double(), G.double(), 1e-12, 1e-14)
            out.update(pfx(truth, key + "truth64/"))
            for j, f in enumerate((0.85, 0.9, 0.95, 1.0, 1.05, 1.1, 1.15)):
                out.update(pfx(grads_of_run(net, y0, t, G, 1e-7 * f, 1e-9), key + "jit%d/" % j))
    save("g12_spread", **out)


# ---------------------------------------------------------------- G14 / G15 (full size, shipped data, the reference itself)
def read_ref_csv_all(path):
    """every time point of the first trajectory of a csvreader-format file (csvreader.py:13-56)"""
    import csv
    with open(path) as fh:
        rows = list(csv.reader(fh))
    dim = int(float(rows[0][0]))
    expr = np.array([[float(v) for v in r if v != ""] for r in rows[1:1 + dim]], np.float32)  # [dim, T]
    tt = np.array([float(v) for v in rows[1 + dim] if v != ""], np.float32)
    assert expr.shape[1] == tt.shape[0]
    return np.ascontiguousarray(expr.T), tt, dim


def g14_g15_fullsize(which=("g14", "g15")):
    """The reference's data-loss half of `training_step` (train_insilico.py:128-132) at the sizes and on the data the
    BASELINE configs name: per-sample `odeint_adjoint(odenet, y0[1,N], t[2], method='dopri5')[1]` over every consecutive
    pair of the shipped sample, loss_data = mean((predictions - target)^2), backward.  Stored: inputs, the reference's own
    ODENet parameters (sparse_ init: 95 % zeros, compresses), predictions, loss, dL/dy0 of every pair, the bias and
    gene-multiplier gradients in full and the three weight gradients at 4 096 fixed positions each."""
    cases = {
        "g14": ("g14_breast11165", "/root/reference/breast_cancer_data/clean_data/desmedt_11165genes_1TESTsample_8middleT.csv", 40, 1411),
        "g15": ("g15_yeast3551", "/root/reference/pramila_yeast_data/clean_data/pramila_3551genes_1sample_24T.csv", 120, 1511),
    }
    torch.set_num_threads(8)
    for key in which:
        name, path, H, seed = cases[key]
        Y, tt, N = read_ref_csv_all(path)
        B = Y.shape[0] - 1
        net = make_net(N, H, seed=seed)                     # reference init (nn.init.sparse_(0.95, std 0.05), g ~ U(0,1))
        for p in net.parameters():
            p.grad = None
        y0s = [torch.from_numpy(Y[i:i + 1].copy()).requires_grad_(True) for i in range(B)]
        target = torch.from_numpy(Y[1:].copy()).reshape(B, 1, N)
        preds = []
        for i in range(B):                                  # the reference's loop, one sample at a time
            preds.append(odeint_adjoint(net, y0s[i], torch.from_numpy(tt[i:i + 2].copy()), method="dopri5")[1])
        predictions = torch.stack(preds)                    # [B, 1, N]
        loss = torch.mean((predictions - target) ** 2)
        loss.backward()
        out = {"Y": Y, "t": tt, "H": np.int32(H), "loss": np.float32(loss.item()),
               "pred": predictions.detach().numpy().reshape(B, N),
               "grad_y0": np.stack([y.grad.numpy().reshape(N) for y in y0s])}
        out.update(pfx(params_np(net), "p_"))
        gr = grads_np(net, "")
        rs = np.random.RandomState(seed)
        for k in ("Ws", "Wp", "Wa"):
            idx = np.sort(rs.choice(gr[k].size, 4096, replace=False)).astype(np.int64)
            out["gidx_" + k] = idx
            out["gval_" + k] = gr[k].reshape(-1)[idx]
            out["gmax_" + k] = np.float32(np.abs(gr[k]).max())   # the tolerance convention normalises by the tensor's max
        for k in ("bs", "bp", "g"):
            out["grad_" + k] = gr[k]
        save(name, **out)
    torch.set_num_threads(1)


if __name__ == "__main__":
    for only, fn in (("--only-g8", "g8_prior"), ("--only-g9", "g9_datahandler"), ("--only-g10", "g10_analysis"),
                     ("--only-g11", "g11_hill"), ("--only-g12", "g12_spread"),
                     ("--only-g13", "g13_hill690"), ("--only-g14", "g14_g15_fullsize"), ("--only-g16", "g16_edges")):
        if only in sys.argv:
            globals()[fn]()
            sys.exit(0)
    g1_g2()
    g3_fixed()
    g4_dopri5()
    g5_training_step()
    g6_controller()
    g7_realdata()
    g8_prior()
    g9_datahandler()
    g10_analysis()
    g11_hill()
    g13_hill690()
    g12_spread()
    g14_g15_fullsize()
    g16_edges()
