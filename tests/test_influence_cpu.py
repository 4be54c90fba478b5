"""CPU-only checks of the gene-influence scoring boundary (phx_influence_scores / phx_influence_workspace_bytes,
include/phoenix_hip.h): the symbols exist, the argument checks answer before any device call, the workspace size is a
plain function of the shape, and the fused callers refuse a CPU network like every other entry point."""
import ctypes as C

import pytest
import torch

from test_abi_cpu import _declared_symbols

BAD_ARG, WORKSPACE = 4, 5


def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_influence_workspace_bytes", "phx_influence_scores"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert lib.phx_abi_version() == 7       # an additive change


def _call(lib, sol=0x1000, T=10, pairs=2, B=3, N=8, genes=(0, 7), scores=0x2000, targets=None, ws=0x3000, ws_bytes=None):
    """phx_influence_scores with made-up device addresses: only calls that must return before touching the device"""
    if ws_bytes is None:
        ws_bytes = max(lib.phx_influence_workspace_bytes(T, pairs, B, N), 1 << 20)
    g = None if genes is None else (C.c_int * len(genes))(*genes)
    return lib.phx_influence_scores(sol, T, pairs, B, N, g, scores, targets, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    _, lib = _lib()
    assert _call(lib, sol=None) == BAD_ARG
    assert _call(lib, scores=None) == BAD_ARG
    assert _call(lib, genes=None) == BAD_ARG
    assert _call(lib, T=1) == BAD_ARG
    assert _call(lib, pairs=0, genes=(0,)) == BAD_ARG
    assert _call(lib, B=0) == BAD_ARG
    assert _call(lib, N=1, genes=(0, 0)) == BAD_ARG
    assert _call(lib, genes=(0, 8)) == BAD_ARG        # N = 8: the last valid index is 7
    assert _call(lib, genes=(-1, 3)) == BAD_ARG
    # a short (or missing) workspace, whether or not targets are asked for
    need = lib.phx_influence_workspace_bytes(10, 2, 3, 8)
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(lib, ws_bytes=need - 1, targets=0x4000) == WORKSPACE
    assert _call(lib, ws=None) == WORKSPACE
    # the argument checks come first
    assert _call(lib, T=1, ws_bytes=0) == BAD_ARG


def test_workspace_bytes_is_positive_and_monotone():
    _, lib = _lib()
    f = lib.phx_influence_workspace_bytes
    assert f(10, 8, 60, 11165) >= 8 * 11165 * 4        # s [pairs, N] lives there when no targets are asked for
    for N in (2, 33, 350, 11165):
        sizes = [f(10, p, 60, N) for p in (1, 2, 3, 8, 40, 1000)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (N, sizes)
    for pairs in (1, 8):
        sizes = [f(10, pairs, 60, N) for N in (2, 3, 4, 97, 350, 2000, 11165, 14691)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (pairs, sizes)
    for shape in ((0, 8, 60, 350), (10, 0, 60, 350), (10, 8, 0, 350), (10, 8, 60, 0), (-1, 8, 60, 350), (10, -3, 60, 350),
                  (10, 8, -60, 350), (10, 8, 60, -350)):
        assert f(*shape) == 0, shape


def test_engine_wrapper_checks_its_arguments():
    from phoenix_amd import engine
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        engine.influence_scores(torch.zeros(10, 12, 8), 2, 3, [0, 1])


@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_fused_callers_have_no_cpu_path(device):
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.gene_influence_matrix(net, 16, "dopri5", n_random_inputs_per_gene=4, device=device, genes=[0, 3])
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.gene_influence_scores(net, 16, "dopri5", n_random_inputs_per_gene=4, device=device, genes=[0, 3],
                                          fused=True)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        phoenix_amd.analysis.gene_influence_matrix(net, 16, "rk4", device=device, genes_per_launch=1)
