"""options={"step_size": h} on the fixed-grid methods: what can be checked without a GPU -- the argument checks of the
Python front end, the two C entry points, and the G17 golden's own consistency."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, relerr

import phoenix_amd
from phoenix_amd import _lib

NEW_SYMBOLS = ("phx_odeint_stepped", "phx_odeint_adjoint_backward_stepped")
HS = (0.5, 0.75, 0.125, 0.3)


@pytest.fixture(scope="module")
def net():
    return phoenix_amd.ODENet("cpu", 12, neurons=4)


def _args(net):
    return net, torch.rand(3, 1, 12), torch.tensor([0.0, 1.0, 2.5])


def test_step_size_reaches_the_device_check(net):
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.odeint(*_args(net), method="rk4", options={"step_size": 0.5})
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.odeint(*_args(net), method="euler", options={"step_size": torch.tensor(0.5)})
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.odeint_adjoint(*_args(net), method="midpoint", options={"step_size": 0.5})


@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf")])
def test_step_size_must_be_positive_and_finite(net, bad):
    with pytest.raises(ValueError, match="step_size"):
        phoenix_amd.odeint(*_args(net), method="rk4", options={"step_size": bad})
    with pytest.raises(ValueError, match="step_size"):
        phoenix_amd.odeint_adjoint(*_args(net), method="rk4", adjoint_options={"step_size": bad})


def test_other_grid_options_stay_unsupported(net):
    for opt in ("grid_constructor", "grid_points", "eps", "first_step", "safety"):
        with pytest.raises(NotImplementedError, match=opt):
            phoenix_amd.odeint(*_args(net), method="rk4", options={opt: 0.5})


def test_adjoint_options_hold_step_size_only(net):
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        phoenix_amd.odeint_adjoint(*_args(net), method="rk4", adjoint_options={"step_size": 0.5})
    with pytest.raises(NotImplementedError, match="adjoint_options"):
        phoenix_amd.odeint_adjoint(*_args(net), method="rk4", adjoint_options={"safety": 0.8})
    with pytest.raises(NotImplementedError, match="adjoint_options"):
        phoenix_amd.odeint_adjoint(*_args(net), method="rk4", adjoint_options={"step_size": 0.5, "safety": 0.8})


def test_dopri5_ignores_step_size_with_the_reference_warning(net):
    with pytest.warns(UserWarning, match="Unexpected arguments"):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.odeint(*_args(net), method="dopri5", options={"step_size": 0.5})


def test_adjoint_dopri5_ignores_its_step_size_with_the_same_warning(net):
    with pytest.warns(UserWarning, match="Unexpected arguments"):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.odeint_adjoint(*_args(net), method="rk4", adjoint_method="dopri5",
                                       adjoint_options={"step_size": 0.5})


def test_new_entry_points_declared_exported_and_null_safe():
    text = open(os.path.join(ROOT, "include", "phoenix_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/phoenix_hip.h"
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.phx_abi_version() == 7
    assert lib.phx_odeint_stepped(None, None, None, 1, 2, None, None, None, None, None, None, 0, None, 0.5) == 4
    assert lib.phx_odeint_adjoint_backward_stepped(None, None, 1, 2, None, None, None, None, None, None, None, None, None,
                                                   0, None, 0.5) == 4


# ---- the golden itself
def test_golden_step_counts():
    g = load_golden("g17_substeps")
    assert tuple(g["hs"]) == HS
    for tname in ("t2", "t5", "t_dec"):
        t = g[tname]
        assert t.dtype == np.float32          # the count is formed in the dtype of t (solvers.py:65)
        count = lambda span, h: int(np.ceil(np.float32(span) / np.float32(h) + np.float32(1))) - 1   # noqa: E731
        for h in (0.5, 0.75, 0.125):          # exactly representable steps: the count is ceil(span / h + 1) - 1
            assert int(g["nsteps/%s/%r" % (tname, h)]) == count(abs(t[-1] - t[0]), h), (tname, h)
            per = [count(abs(t[i] - t[i - 1]), h) for i in range(len(t) - 1, 0, -1)]
            assert g["nsteps_bwd/%s/%r" % (tname, h)].tolist() == per, (tname, h)
    assert int(g["nsteps/t5/0.125"]) == 72 and int(g["nsteps/t2/0.75"]) == 3 and int(g["nsteps/t_dec/0.75"]) == 2
    assert g["ps/nsteps"].tolist() == [math.ceil((0.4 + 0.33 * b) / 0.25 + 1) - 1 for b in range(5)]


@pytest.mark.parametrize("yname", ["single", "batch"])
def test_golden_small_steps_approach_the_truth(yname):
    g17, g3 = load_golden("g17_substeps"), load_golden("g3_fixed")
    truth = g17["truth64/" + yname]
    fine = relerr(g17["rk4/t5/0.125/%s/sol" % yname], truth)
    one_step = relerr(g3["rk4/t5/%s/sol" % yname], truth)
    assert fine < one_step, (fine, one_step)
    assert np.array_equal(g17["y0_" + yname], g3["y0_" + yname]) and np.array_equal(g17["p_Ws"], g3["p_Ws"])
