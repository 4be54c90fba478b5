"""Golden G25 (tests/golden/g25_dopri5_truth*.npz): what its generator (tests/golden/make_golden_truth.py), the CPU test
(test_oracle_vs_golden.py) and the GPU test (test_dopri5_truth_gpu.py) share -- the cases, the seeded inputs (drawn here,
never stored: at N = 1100 the parameters would not fit; the golden holds their checksums), the error measures and the bar.

The bar (nothing in it comes from the code under test; the factors are golden G12's, test_gpu_parity.py):
  per case and mode   worst gradient error against the fp64 truth <= 1.5 x the largest of the reference's own seven
                      (its fp32 runs at rtol x {0.85 ... 1.15}); the same for the worst per-row dL/dy0 error
  per regime          median over the regime's cases and modes <= 1.25 x the reference's median
"""
import numpy as np

KEYS = ("Ws", "bs", "Wp", "bp", "Wa", "g")
WEIGHTS = ("Ws", "Wp", "Wa")
GRADS = ("y0",) + KEYS
JITTER = (0.85, 0.9, 0.95, 1.0, 1.05, 1.1, 1.15)
NPOS = 4096
WORST, MEDIAN = 1.5, 1.25

# (N, H, B), regime of the cotangents, kernel family (phx_debug_*_kernel_m), HC = hidden chunks, Hc = rows per chunk
CASES = (
    ((1100, 40, 5), "unit", 3, 1, 40),
    ((1100, 48, 19), "train", 3, 1, 48),
    ((70, 49, 19), "train", 4, 2, 25),
    ((70, 96, 19), "unit", 4, 2, 48),
    ((70, 97, 19), "train", 4, 3, 33),
    ((70, 145, 5), "unit", 4, 4, 37),
    ((70, 193, 5), "train", 4, 5, 39),
    ((70, 241, 5), "unit", 4, 6, 41),
    ((70, 256, 19), "unit", 4, 6, 43),
    ((330, 49, 80), "train", 4, 2, 25),
)
SHAPES = tuple(c[0] for c in CASES)
MULTI = ((1100, 40, 5), (70, 97, 19))          # also solved on t = [0, 0.4, 1] with a cotangent at the inner time
T2 = np.array([0.0, 1.0], np.float32)
T3 = np.array([0.0, 0.4, 1.0], np.float32)
# (shape, mode): "shared" = one batched call, "per" = one call per trajectory, "multi" = shared control on T3
RUNS = tuple((s, m) for s in SHAPES for m in ("shared", "per")) + tuple((s, "multi") for s in MULTI)


def name(shape, mode):
    return "n%d_h%d_b%d/%s/" % (shape + (mode,))


def regime(shape):
    return CASES[SHAPES.index(shape)][1]


def params(N, H, seed, std=0.05, neg=0.1):
    r = np.random.RandomState(seed)
    g = r.rand(N).astype(np.float32)
    g[r.rand(N) < neg] *= -1
    return {"Ws": (r.randn(H, N) * std).astype(np.float32), "bs": r.uniform(-.2, .2, H).astype(np.float32),
            "Wp": (r.randn(H, N) * std).astype(np.float32), "bp": r.uniform(-.2, .2, H).astype(np.float32),
            "Wa": (r.randn(N, 2 * H) * std).astype(np.float32), "g": g}


def checksums(p):
    """[6, 2] float64: sum and sum of squares of every parameter array"""
    return np.array([[np.sum(p[k], dtype=np.float64), np.sum(p[k].astype(np.float64) ** 2)] for k in KEYS])


def inputs(shape, mode):
    """parameters, y0 [B, N], t [T] and the cotangent of the solution G [T, B, N] (zero at t[0])"""
    N, H, B = shape
    seed = 2500 + SHAPES.index(shape)
    p = params(N, H, seed)
    r = np.random.RandomState(seed + 100)
    y0 = np.clip(0.15 * r.randn(B, N) + 0.5, 0.03, 1.07).astype(np.float32)
    t = T3 if mode == "multi" else T2
    G = np.zeros((3, B, N))
    G[1:] = r.randn(2, B, N)                 # G[2]: the end, G[1]: the inner time of T3 -- drawn for every mode alike
    G = G[[0, 2]] if mode != "multi" else G
    if regime(shape) == "train":
        G /= B * N
    elif mode == "per":
        G *= (10.0 ** -(np.arange(B) % 3))[None, :, None]     # rows of different size: see errors()
    return p, y0, t, G.astype(np.float32)


def positions(shape, k):
    """where a weight gradient is stored: 4 096 fixed positions (golden G14's convention), or all of a smaller one"""
    N, H, B = shape
    size = 2 * H * N if k == "Wa" else H * N
    if size <= NPOS:
        return np.arange(size)
    r = np.random.RandomState(25000 + SHAPES.index(shape) * 3 + WEIGHTS.index(k))
    return np.sort(r.choice(size, NPOS, replace=False))


def stored(shape, grads):
    """a run's gradients {y0, Ws ... g} as the golden stores them: weights at positions() with the tensor's max"""
    out = {}
    for k in GRADS:
        a = np.asarray(grads[k], np.float64)
        if k in WEIGHTS:
            out[k] = a.reshape(-1)[positions(shape, k)]
            out["max_" + k] = np.float64(np.abs(a).max())
        else:
            out[k] = a.reshape(-1, shape[0]) if k == "y0" else a.reshape(-1)
    return out


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - b))) / max(float(np.max(np.abs(b))), 1e-30)


def errors(got, truth, rel=_rel):
    """got, truth: stored() forms.  One error per gradient under the suite's relerr (`rel`) -- max |a - b| / max |b|, the
    max of a weight gradient being that of the whole tensor: the truth's max is appended to both sides -- plus "row": the
    worst dL/dy0 row, each row normalised by its OWN truth maximum (relerr passes a row that is wrong at 1e-3 if the row
    is small)."""
    e = {}
    for k in GRADS:
        a, b = np.asarray(got[k], np.float64), np.asarray(truth[k], np.float64)
        if k in WEIGHTS:
            a, b = np.append(a, truth["max_" + k]), np.append(b, truth["max_" + k])
        e[k] = rel(a, b)
    e["row"] = max(_rel(a, b) for a, b in zip(got["y0"], truth["y0"]))
    return e


def worst(e):
    return max(e[k] for k in GRADS)


def load():
    """the golden (both files: a committed file stays under 1 MiB) as one dict"""
    from conftest import load_golden
    d = load_golden("g25_dopri5_truth")
    d.update(load_golden("g25_dopri5_truth_w"))
    return d


def truth_of(gold, shape, mode):
    """the stored truth of a run; a "per" run of the training-scale regime is the problem of its "shared" run"""
    pre = name(shape, "shared" if mode == "per" and regime(shape) == "train" else mode) + "truth/"
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


def checksums_of(gold, shape):
    return gold["n%d_h%d_b%d/checksums" % shape]


def reference_errors(gold, shape, mode):
    """[7, 8] the reference's fp32 errors at rtol x JITTER: columns GRADS + ("row",)"""
    return gold[name(shape, mode) + "ref_err"]


def bars(gold, shape, mode):
    """(bar of the worst gradient error, bar of the per-row figure, the reference's seven worst-gradient errors)"""
    r = reference_errors(gold, shape, mode)
    per_run = r[:, :len(GRADS)].max(1)
    return WORST * float(per_run.max()), WORST * float(r[:, len(GRADS)].max()), per_run


def table_line(tag, shape, mode, e, gold):
    b, brow, per_run = bars(gold, shape, mode)
    return "%-10s %-18s %-6s %-5s worst %.2e (bar %.2e) row %.2e (bar %.2e) | %s" % (
        tag, "%d/%d/%d" % shape, mode, regime(shape), worst(e), b, e["row"], brow,
        " ".join("%s %.1e" % (k, e[k]) for k in GRADS))
