"""CPU-only checks of the per-gene neighbour lists (phx_effects_neighbors / phx_effects_neighbors_workspace_bytes,
include/phoenix_hip.h; `effects_neighbors`, `write_link_list`): `neighbors_ref`, the numpy restatement on a dense matrix that
tests/test_neighbors_gpu.py holds the kernel to, is pinned to a brute-force loop and, through the fixture g23_neighbors.npz
(tests/golden/make_golden_neighbors.py), to the reference's own ranked list `get_link_list`; `write_link_list` reproduces the
reference's file; the symbols exist, and the argument checks answer before any device call."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_cpu import _declared_symbols
from test_edges_cpu import select_ref

BAD_ARG, WORKSPACE = 4, 5
ORIENT, DIAGONAL = 1, 2
OF_REGULATOR, OF_TARGET = 0, 1


def neighbors_ref(M, k, of="target", regulators=None, targets=None, threshold=None, orient=False, diagonal=False):
    """(gene int64 [N, k], value float32 [N, k], count int64 [N], s64 float64 [N]) of the float32 matrix M [N, N] (regulator
    row, target column).  Eligible is what `select_ref` (tests/test_edges_cpu.py) selects -- finite, non-zero, off the diagonal
    unless `diagonal`, with `orient` |M[i,j]| > |M[j,i]| strictly, |M| >= threshold -- with its regulator in `regulators` and
    its target in `targets` (None: all).  Line n is column n (of="target") or row n (of="regulator"); its entries are ordered
    by magnitude descending, then by the other gene's index; padding is gene -1, value +0.  s64 is the float64 sum of the
    float32 magnitudes of the line's eligible entries."""
    M = np.asarray(M)
    N = M.shape[0]
    assert of in ("target", "regulator")
    i, j, v = select_ref(M, threshold=1e-45 if threshold is None else threshold, orient=orient, diagonal=diagonal)
    keep = np.ones(len(v), bool)
    if regulators is not None:
        keep &= np.isin(i, np.asarray(list(regulators), np.int64))
    if targets is not None:
        keep &= np.isin(j, np.asarray(list(targets), np.int64))
    i, j, v = i[keep], j[keep], v[keep]
    line, other = (j, i) if of == "target" else (i, j)
    gene = np.full((N, k), -1, np.int64)
    value = np.zeros((N, k), np.float32)
    count = np.zeros(N, np.int64)
    s64 = np.zeros(N, np.float64)
    for n in range(N):
        sel = np.nonzero(line == n)[0]
        # select_ref's order is magnitude descending, then (i, j): inside one line that is the other gene ascending
        count[n] = len(sel)
        s64[n] = np.abs(v[sel]).astype(np.float64).sum()
        sel = sel[:k]
        gene[n, :len(sel)] = other[sel]
        value[n, :len(sel)] = v[sel]
    return gene, value, count, s64


def brute_force(M, k, of, regulators, targets, threshold, orient, diagonal):
    """the definition, entry by entry in plain Python"""
    N = M.shape[0]
    gene = np.full((N, k), -1, np.int64)
    value = np.zeros((N, k), np.float32)
    count = np.zeros(N, np.int64)
    for n in range(N):
        found = []
        for o in range(N):
            i, j = (o, n) if of == "target" else (n, o)
            a, b = float(M[i, j]), float(M[j, i])
            if not np.isfinite(a) or a == 0:
                continue
            if orient:
                if i == j or np.isnan(b) or not abs(a) > abs(b):
                    continue
            elif i == j and not diagonal:
                continue
            if regulators is not None and i not in regulators:
                continue
            if targets is not None and j not in targets:
                continue
            if threshold is not None and not abs(a) >= threshold:
                continue
            found.append((-abs(a), o, M[i, j]))
        found.sort(key=lambda t: (t[0], t[1]))
        count[n] = len(found)
        for r, (_, o, v) in enumerate(found[:k]):
            gene[n, r], value[n, r] = o, v
    return gene, value, count


def same_lists(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32)) and
            np.array_equal(a[2], b[2]))


# --------------------------------------------------------------------------- the restatement against the definition
def test_neighbors_ref_equals_a_brute_force_loop():
    rng = np.random.default_rng(5)
    cases = 0
    for N in (5, 9, 14):
        M = (rng.integers(-6, 7, size=(N, N)) / 4.0).astype(np.float32)        # ties and zeros abound
        M[rng.integers(0, N), rng.integers(0, N)] = np.nan
        M[rng.integers(0, N), rng.integers(0, N)] = np.inf
        M[rng.integers(0, N), rng.integers(0, N)] = -np.inf
        M[0, 1] = -0.0
        regs = sorted(set(rng.integers(0, N, size=N).tolist()))
        tgts = sorted(set(rng.integers(0, N, size=N).tolist()))
        for of in ("target", "regulator"):
            for orient in (False, True):
                for diagonal in (False, True):
                    for regulators, targets in ((None, None), (regs, None), (None, tgts), (regs + regs[:1], tgts)):
                        for threshold in (None, 0.75, 0.8):
                            for k in (1, 3, N + 2):
                                kw = dict(of=of, regulators=regulators, targets=targets, threshold=threshold, orient=orient,
                                          diagonal=diagonal)
                                ref = neighbors_ref(M, k, **kw)
                                assert same_lists(ref[:3], brute_force(M, k, **kw)), (N, k, kw)
                                assert np.all(np.signbit(ref[1][ref[0] < 0]) == 0)
                                cases += 1
    print("neighbors_ref equals the brute-force loop in %d cases" % cases)


def grouped(reg, tgt, score, N, k, of):
    """the reference's ranked list grouped by target (or regulator), the first k of every group"""
    gene = np.full((N, k), -1, np.int64)
    mag = np.zeros((N, k), np.float32)
    count = np.zeros(N, np.int64)
    line, other = (tgt, reg) if of == "target" else (reg, tgt)
    for n, o, s in zip(line.tolist(), other.tolist(), score):
        if count[n] < k:
            gene[n, count[n]], mag[n, count[n]] = o, s
        count[n] += 1
    return gene, mag, count


def golden_cases():
    g = load_golden("g23_neighbors")
    e = load_golden("g21_edges")
    for tag, M in (("plain", e["effects"]), ("masked", e["masked"])):
        for ctag, cand in (("all", None), ("cand", g["candidates"].tolist())):
            yield tag, ctag, M, cand, tuple(g["%s_%s_%s" % (tag, ctag, x)] for x in ("regulator", "target", "score"))


def test_neighbors_ref_reproduces_the_reference_ranking():
    g = load_golden("g23_neighbors")
    assert g["candidates"].tolist() == [i for i in range(37) if i % 3 != 0]
    n = 0
    for tag, ctag, M, cand, (reg, tgt, score) in golden_cases():
        N = M.shape[0]
        assert np.array_equal(score, np.abs(M)[reg, tgt]) and np.all(score > 0)
        for of in ("target", "regulator"):
            for k in (1, 5, 64):
                gene, mag, count = grouped(reg, tgt, score, N, k, of)
                # `masked` is make_mask of `effects`: the plain selection on it and the oriented one on `effects` agree
                refs = [neighbors_ref(M, k, of=of, regulators=cand)]
                if tag == "masked":
                    refs.append(neighbors_ref(load_golden("g21_edges")["effects"], k, of=of, regulators=cand, orient=True))
                for ref in refs:
                    assert np.array_equal(ref[0], gene) and np.array_equal(np.abs(ref[1]), mag) and np.array_equal(ref[2], count), \
                        (tag, ctag, of, k)
                    n += 1
    print("G23: %d groupings of the reference's ranked list equal neighbors_ref" % n)


# --------------------------------------------------------------------------- the link-list writer
def test_write_link_list_reproduces_the_reference_file(tmp_path):
    import phoenix_amd
    names = ["g%d" % i for i in range(37)]
    g = load_golden("g23_neighbors")
    for tag, ctag, M, cand, (reg, tgt, score) in golden_cases():
        text = str(g["%s_%s_text" % (tag, ctag)])
        assert text.count("\n") == 40
        value = M[reg[:40], tgt[:40]]                                       # signed, as the kernel reports them
        edges = phoenix_amd.Edges(torch.from_numpy(reg[:40]), torch.from_numpy(tgt[:40]), torch.from_numpy(value))
        path = os.path.join(str(tmp_path), "links_%s_%s.txt" % (tag, ctag))
        assert phoenix_amd.write_link_list(path, edges, gene_names=names) == 40
        assert open(path).read() == text, (tag, ctag)
        buf = io.StringIO()
        phoenix_amd.write_link_list(buf, edges)
        want = "".join("G%d\tG%d\t%.6f\n" % (i + 1, j + 1, s) for i, j, s in zip(reg[:40], tgt[:40], score[:40]))
        assert buf.getvalue() == want
        buf = io.StringIO()
        phoenix_amd.write_link_list(buf, edges, gene_names=names, signed=True)
        assert buf.getvalue() == "".join("g%d\tg%d\t%.6f\n" % (i, j, v) for i, j, v in zip(reg[:40], tgt[:40], value))
    assert (value < 0).any()


def test_write_link_list_of_neighbors_skips_the_padding():
    import phoenix_amd
    M = load_golden("g21_edges")["effects"]
    for of in ("target", "regulator"):
        gene, value, count, s64 = neighbors_ref(M, 40, of=of)
        assert (gene < 0).any()
        nb = phoenix_amd.Neighbors(torch.from_numpy(gene), torch.from_numpy(value), torch.from_numpy(count),
                                   torch.from_numpy(s64.astype(np.float32)))
        buf = io.StringIO()
        n = phoenix_amd.write_link_list(buf, nb, of=of)
        want = []
        for line in range(M.shape[0]):
            for r in range(40):
                if gene[line, r] >= 0:
                    i, j = (gene[line, r], line) if of == "target" else (line, gene[line, r])
                    want.append("G%d\tG%d\t%.6f\n" % (i + 1, j + 1, abs(float(value[line, r]))))
        assert n == len(want) == int(np.minimum(count, 40).sum()) and buf.getvalue() == "".join(want)
        with pytest.raises(ValueError, match="write_link_list"):
            phoenix_amd.write_link_list(io.StringIO(), nb)
    with pytest.raises(ValueError, match="write_link_list"):
        phoenix_amd.write_link_list(io.StringIO(), (gene, value))
    with pytest.raises(ValueError, match="write_link_list"):
        phoenix_amd.write_link_list(io.StringIO(), nb, gene_names=["a", "b"], of="target")


# --------------------------------------------------------------------------- the C boundary
def _lib():
    from phoenix_amd import _lib
    return _lib, _lib.load()


def test_both_symbols_are_exported_and_declared():
    mod, lib = _lib()
    for name in ("phx_effects_neighbors_workspace_bytes", "phx_effects_neighbors"):
        assert name in mod.EXPORTS and name in _declared_symbols() and hasattr(lib, name), name
    assert set(mod.EXPORTS) == set(_declared_symbols())
    assert lib.phx_abi_version() == 7       # an additive change
    assert mod.NEIGHBORS_AXES == {"regulator": OF_REGULATOR, "target": OF_TARGET} and mod.NEIGHBORS_MAX_K == 64
    import phoenix_amd
    assert phoenix_amd.effects_neighbors is phoenix_amd.analysis.effects_neighbors
    assert phoenix_amd.write_link_list is phoenix_amd.analysis.write_link_list
    assert phoenix_amd.Neighbors._fields == ("gene", "value", "count", "strength")


def test_the_unit_is_listed_and_its_listing_exists():
    from phoenix_amd import build
    assert "phx_neighbors.hip" in build.LISTINGS
    src = [s for s in build.sources() if os.path.basename(s) == "phx_neighbors.hip"]
    assert len(src) == 1 and os.path.exists(build.listing_of(src[0]))


def _params(mod, N=8, H=3, **null):
    """phx_params with made-up device addresses"""
    addr = {"Ws": 0x1000, "bs": 0x2000, "Wp": 0x3000, "bp": 0x4000, "WaT": 0x5000, "g": 0x6000}
    addr.update(null)
    return mod.PhxParams(addr["Ws"], addr["bs"], addr["Wp"], addr["bp"], addr["WaT"], addr["g"], N, H, None)


def _call(mod, lib, p="default", mode=2, y=0x7000, ph=0x8000, B=3, flags=ORIENT, axis=OF_TARGET, k=5, tau=0.5, rok=0x9000,
          tok=None, gene=0xa000, value=0xb000, count=0xc000, strength=0xd000, ws=0xe000, ws_bytes=1 << 30):
    """phx_effects_neighbors with made-up device addresses: only calls that must return before touching the device"""
    if p == "default":
        p = _params(mod)
    return lib.phx_effects_neighbors(None if p is None else C.byref(p), mode, y, ph, B, flags, axis, k, tau, rok, tok, gene,
                                     value, count, strength, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_gpu():
    mod, lib = _lib()
    assert _call(mod, lib, p=None) == BAD_ARG
    for name in ("Ws", "Wp", "WaT", "g"):
        assert _call(mod, lib, p=_params(mod, **{name: None})) == BAD_ARG, name
    for bad in (dict(N=1), dict(N=0), dict(N=-8), dict(N=65536), dict(H=0), dict(H=257), dict(H=-1)):
        assert _call(mod, lib, p=_params(mod, **bad)) == BAD_ARG, bad
    for mode in (-1, 3, 7):
        assert _call(mod, lib, mode=mode) == BAD_ARG, mode
    for mode in (1, 2):                                    # the Jacobian modes need their states
        for bad in (dict(y=None), dict(ph=None), dict(B=0), dict(B=-2)):
            assert _call(mod, lib, mode=mode, **bad) == BAD_ARG, bad
    for flags in (-1, 4, 8, 7):
        assert _call(mod, lib, flags=flags) == BAD_ARG, flags
    for axis in (-1, 2, 5):
        assert _call(mod, lib, axis=axis) == BAD_ARG, axis
    for k in (0, -1, 65, 1000):
        assert _call(mod, lib, k=k) == BAD_ARG, k
    for tau in (-0.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e39):
        assert _call(mod, lib, tau=tau) == BAD_ARG, tau
    for name in ("gene", "value", "count", "strength"):
        assert _call(mod, lib, **{name: None}) == BAD_ARG, name
    # every argument in order: the workspace is asked for next (tau = +0 is "no threshold", a subnormal is positive)
    need = lib.phx_effects_neighbors_workspace_bytes(8, 3, 3, 2, OF_TARGET, 5)
    assert need > 0
    for kw in (dict(), dict(tau=0.0), dict(tau=1e-45), dict(k=1), dict(axis=OF_REGULATOR), dict(rok=None), dict(flags=0)):
        assert _call(mod, lib, ws=None, **kw) == WORKSPACE, kw
    assert _call(mod, lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(mod, lib, k=64, ws_bytes=need) == WORKSPACE                  # the lists grow with k


def test_workspace_bytes(monkeypatch):
    _, lib = _lib()
    f = lib.phx_effects_neighbors_workspace_bytes
    assert f.restype is C.c_size_t
    monkeypatch.delenv("PHX_NEIGHBORS_SEGMENTS", raising=False)
    for args in ((1, 40, 3, 2, 1, 5), (0, 40, 3, 2, 1, 5), (65536, 40, 3, 2, 1, 5), (350, 0, 3, 2, 1, 5), (350, 257, 3, 2, 1, 5),
                 (350, 40, 0, 2, 1, 5), (350, 40, 0, 1, 1, 5), (350, 40, 3, 5, 1, 5), (350, 40, 3, -1, 1, 5), (350, 40, 3, 2, 2, 5),
                 (350, 40, 3, 2, -1, 5), (350, 40, 3, 2, 1, 0), (350, 40, 3, 2, 1, 65)):
        assert f(*args) == 0, args
    # every served H, mode, axis and k: the selection never refuses a combination, whatever the image takes of the LDS
    for H in (1, 40, 224, 225, 256):
        for mode in (0, 1, 2):
            for axis in (0, 1):
                for k in (1, 20, 64):
                    assert f(11165, H, 60, mode, axis, k) > 0, (H, mode, axis, k)
    # S segments of 64-gene line tiles, k keys of 8 bytes, a count and a sum per line: 130 genes are 3 tiles, one segment each
    per_segment = lambda k: 192 * k * 8 + 2 * 192 * 4                                        # noqa: E731
    assert per_segment(5) * 3 <= f(130, 40, 2, 2, 1, 5) <= per_segment(5) * 3 + 3 * 256
    assert f(350, 40, 0, 0, 1, 5) == f(350, 40, -7, 0, 0, 5) > 0                             # effects ignores B
    sizes = []
    for s in ("1", "2", "3", "100"):
        monkeypatch.setenv("PHX_NEIGHBORS_SEGMENTS", s)
        sizes.append(f(130, 40, 2, 2, 1, 5))
    assert sizes[0] < sizes[1] < sizes[2] == sizes[3]                                        # at most one segment per tile


# --------------------------------------------------------------------------- the Python caller
def test_python_caller_refuses_bad_arguments_and_a_cpu_network():
    import phoenix_amd
    net = phoenix_amd.ODENet("cpu", 16, neurons=4)
    y = torch.rand(3, 16)
    for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(k=2.5), dict(k=True), dict(k="7"), dict(k=None),
               dict(k=5, of="targets"), dict(k=5, of="row"), dict(k=5, of=None), dict(k=5, of=1),
               dict(k=5, regulators=[0, 16]), dict(k=5, regulators=[-1]), dict(k=5, targets=[3, 99]), dict(k=5, targets=[-2, 1]),
               dict(k=5, regulators=torch.tensor([0, 16])), dict(k=5, targets=np.array([16])),
               dict(k=5, regulators=[0.5, 1.0]), dict(k=5, targets=[[1, 2]]), dict(k=5, regulators="abc"),
               dict(k=5, threshold=0.0), dict(k=5, threshold=-1.0), dict(k=5, threshold=float("inf")),
               dict(k=5, threshold=float("nan")), dict(k=5, threshold="1"), dict(k=5, threshold=True)):
        with pytest.raises(ValueError, match="effects_neighbors"):
            phoenix_amd.effects_neighbors(net, **kw)
        with pytest.raises(ValueError, match="effects_neighbors"):
            phoenix_amd.effects_neighbors(net, y=y, **kw)
    for reduce in ("sum", "abs", None, "effects", 1):
        with pytest.raises(ValueError, match="reduce"):
            phoenix_amd.effects_neighbors(net, 5, y=y, reduce=reduce)
    for kw in (dict(), dict(of="regulator"), dict(regulators=[1, 1, 2], targets=torch.tensor([0, 15])), dict(threshold=0.1),
               dict(y=y), dict(orient=True, diagonal=True), dict(regulators=[], targets=())):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            phoenix_amd.effects_neighbors(net, 5, **kw)
