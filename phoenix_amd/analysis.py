"""Row f3 of SURVEY.md section 8: the batched analysis callers of the hot path.

`gene_influence_scores` is the loop of find_gene_influences.py:64-77 (per gene: integrate a random batch of initial
states, overwrite that gene's column with a second random draw, integrate again, score = mean |difference| over all
OTHER genes and all projected time points after the first).  Every solve keeps the reference's batch semantics (one
shared adaptive step size per `odeint` call of the `[n_inputs, 1, N]` batch, 10 interpolated outputs on a float64
grid), but the two solves of `genes_per_launch` genes go to the engine together (`odeint_calls`: one batch group and
one step controller per call, as many calls per launch as the device holds) and the scores stay on the device until
the end (the reference calls `.item()` inside the loop).
`fused=True` and `gene_influence_matrix` keep the scoring on the device as well: draws and perturbed copies are written
straight into one initial-state buffer, the solver's output block is scored by one pass of phx_influence_scores
(include/phoenix_hip.h) instead of six small launches per gene, and the per-target means that pass computes anyway are
the gene -> gene influence matrix.
`DataHandler.calculate_trajectory` (phoenix_amd/data.py) is the other caller of this row.
"""
import collections

import numpy as np
import torch

from . import engine
from .odeint import _calls_block, odeint_calls
from .odenet import params_of


def influence_score(unpert_out, pert_out, this_gene):
    """find_gene_influences.py:74-75: mean over outputs 1.., samples and every gene but `this_gene`."""
    diff = (unpert_out[1:] - pert_out[1:]).abs()
    n_other = diff.shape[-1] - 1
    total = diff.sum() - diff[..., this_gene].sum()
    return total / (diff[..., 0].numel() * n_other)


def gene_influence_scores(odenet, dim, method, n_random_inputs_per_gene=60, time_pts_to_project=None, device="cuda",
                          genes=None, draws=None, genes_per_launch=8, fused=False):
    """Returns a float32 numpy array with one score per gene in `genes` (default: all `dim` genes, in order).
    `draws(gene) -> (this_init [n,1,dim], this_pert_col [n])` replaces the reference's two `torch.rand` calls
    (find_gene_influences.py:69,71); by default they are drawn on `device` in the same order.
    `fused=True`: the same scan with the scoring in one kernel pass per launch (`gene_influence_matrix` without the
    matrix); it differs from the default path in the order of the sums only."""
    if fused:
        return _fused_scan(odenet, dim, method, n_random_inputs_per_gene, time_pts_to_project, device, genes, draws,
                           genes_per_launch, want_matrix=False)[0]
    if time_pts_to_project is None:
        time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))              # :65 (float64 grid)
    t = time_pts_to_project.to(device)
    genes = list(range(dim)) if genes is None else list(genes)
    scores = torch.zeros(len(genes), dtype=torch.float32, device=device)
    with torch.no_grad():
        for k0 in range(0, len(genes), genes_per_launch):
            batch = genes[k0:k0 + genes_per_launch]
            inits = []
            for this_gene in batch:
                if draws is None:
                    this_init = 1 * (torch.rand(n_random_inputs_per_gene, 1, dim, device=device) - 0.5)
                    this_pert_col = 1 * (torch.rand(n_random_inputs_per_gene, device=device) - 0.5)
                else:
                    this_init, this_pert_col = (x.to(device) for x in draws(this_gene))
                pert_init = this_init.clone()
                pert_init[:, 0, this_gene] = this_pert_col
                inits += [this_init, pert_init]
            out = odeint_calls(odenet, torch.stack(inits), t, method=method)   # [2k, T, n, 1, dim]
            for j, this_gene in enumerate(batch):
                scores[k0 + j] = influence_score(out[2 * j], out[2 * j + 1], this_gene)
    return scores.cpu().numpy()


def gene_influence_matrix(odenet, dim, method, n_random_inputs_per_gene=60, time_pts_to_project=None, device="cuda",
                          genes=None, draws=None, genes_per_launch=8):
    """The scan of `gene_influence_scores(fused=True)` with what it discards: returns (scores [G] float32 numpy,
    matrix [G, dim] float32 tensor on `device`), G = len(genes).  matrix[i, n] = mean over the projected time points
    after the first and over the random inputs of |unperturbed - perturbed| of target gene n when genes[i] is
    perturbed; scores[i] is the mean of row i over n != genes[i] (find_gene_influences.py:74-75).  The diagonal entry
    matrix[i, genes[i]] (the perturbed gene itself) is reported as computed and left out of the score only.  Same draws
    in the same order as `gene_influence_scores`."""
    return _fused_scan(odenet, dim, method, n_random_inputs_per_gene, time_pts_to_project, device, genes, draws,
                       genes_per_launch, want_matrix=True)


def _fused_scan(odenet, dim, method, n, time_pts_to_project, device, genes, draws, genes_per_launch, want_matrix):
    engine._require_gpu(params_of(odenet)[0], "odenet")
    if time_pts_to_project is None:
        time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))              # :65 (float64 grid)
    t = time_pts_to_project.to(device)
    genes = list(range(dim)) if genes is None else [int(g) for g in genes]
    k_max = max(1, min(int(genes_per_launch), len(genes)))
    scores = torch.empty(len(genes), dtype=torch.float32, device=device)
    matrix = torch.empty((len(genes), dim), dtype=torch.float32, device=device) if want_matrix else None
    y0s = torch.empty((2 * k_max, n, 1, dim), dtype=torch.float32, device=device)
    with torch.no_grad():
        for k0 in range(0, len(genes), k_max):
            batch = genes[k0:k0 + k_max]
            for j, this_gene in enumerate(batch):
                init, pert = y0s[2 * j], y0s[2 * j + 1]
                if draws is None:     # the two torch.rand calls of :69,71, in that order, into place
                    torch.rand((n, 1, dim), out=init)
                    init.sub_(0.5)
                    col = torch.rand(n, device=device) - 0.5
                else:
                    this_init, col = draws(this_gene)
                    init.copy_(this_init)
                pert.copy_(init)
                pert[:, 0, this_gene] = col
            sol = _calls_block(odenet, y0s[:2 * len(batch)], t, method=method)      # [T, 2k*n, dim]
            engine.influence_scores(sol, len(batch), n, batch, scores=scores[k0:k0 + len(batch)],
                                    targets=matrix[k0:k0 + len(batch)] if want_matrix else None)
            del sol       # one output block alive at a time
    return scores.cpu().numpy(), matrix


KnockoutEffects = collections.namedtuple("KnockoutEffects", ("genes", "scores", "shift", "magnitude"))


def _screen_setup(name, odenet, y0, time_pts_to_project, N, host_check=None):
    """What a knockout screen does between its argument checks and its first solve: the y0 check, host_check(T, B) -- the
    caller's ValueErrors that need the grid -- and only then the GPU requirement on the model and y0
    -> (y0 [B, 1, N] detached, the time grid on y0's device; default the scan's float64 arange(0, 1, 0.1))"""
    if y0.shape[-1] != N or y0.dim() not in (2, 3) or y0.dtype != torch.float32:
        raise ValueError("%s: y0 must be float32 [B, 1, %d] or [B, %d], got %s %s" % (name, N, N, y0.dtype, tuple(y0.shape)))
    if time_pts_to_project is None:
        time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))
    if host_check is not None:
        host_check(int(time_pts_to_project.shape[-1]), y0.numel() // N)
    engine._require_gpu(params_of(odenet)[0], "odenet")
    engine._require_gpu(y0, "y0")
    return y0.detach().reshape(-1, 1, N), time_pts_to_project.to(y0.device)


def _knockout_args(N, genes, value, genes_per_launch):
    """(genes, values) of `knockout_effects` as lists of G ints / floats, checked on the host before any launch"""
    genes = list(range(N)) if genes is None else engine.int_list("knockout_effects", genes)
    engine.check_genes("knockout_effects", genes, N)
    if not genes:
        raise ValueError("knockout_effects: no gene to clamp")
    values = engine.gene_values("knockout_effects", value, len(genes))
    if not hasattr(genes_per_launch, "__index__") or int(genes_per_launch) < 1:
        raise ValueError("knockout_effects: genes_per_launch must be a positive integer")
    return genes, values


def knockout_effects(odenet, y0, genes=None, value=0.0, time_pts_to_project=None, method="dopri5", genes_per_launch=8,
                     want_matrices=True):
    """In-silico knockout / over-expression screen: what does the system do when gene g is HELD at `value` for the whole
    time course?  (`gene_influence_scores` nudges only the initial value, which relaxes back under the gene's own dynamics.)
    y0 [B, 1, N] or [B, N]: the states to start from (data states, or `rand - 0.5` like the scan); genes: the G genes to
    clamp, one at a time (default: all N); value: a scalar or [G] levels, 0 a knockout, a large level an over-expression;
    time_pts_to_project: default the scan's arange(0, 1, 0.1).
    The unperturbed solve runs once.  Per block of `genes_per_launch` genes, call k starts from y0 with column genes[k]
    set to value[k] and integrates with d y[:, genes[k]] / dt = 0 (`odeint_calls(clamp=...)`), and one pass of
    phx_knockout_effects scores the block against the baseline; one output block is alive at a time.
    Returns KnockoutEffects(genes, scores [G] float32 numpy, shift [G, N], magnitude [G, N] device tensors or None):
    with d = clamped - baseline over the projected time points after the first and the B states, shift[i, n] is the mean
    of d (signed: target n goes up or down), magnitude[i, n] the mean of |d|, scores[i] the mean of magnitude[i, n] over
    n != genes[i] -- a per-gene vector like the influence scores, for `consolidate_gene_scores` and
    `pathway_permutation_test` as it is."""
    N = params_of(odenet)[0].shape[1]
    genes, values = _knockout_args(N, genes, value, genes_per_launch)      # first: refused whatever else holds
    y0, t = _screen_setup("knockout_effects", odenet, y0, time_pts_to_project, N)
    device = y0.device
    B, G = y0.shape[0], len(genes)
    k_max = max(1, min(int(genes_per_launch), G))
    scores = torch.empty(G, dtype=torch.float32, device=device)
    shift = torch.empty((G, N), dtype=torch.float32, device=device) if want_matrices else None
    magnitude = torch.empty((G, N), dtype=torch.float32, device=device) if want_matrices else None
    y0s = torch.empty((k_max, B, 1, N), dtype=torch.float32, device=device)
    with torch.no_grad():
        base = _calls_block(odenet, y0.unsqueeze(0), t, method=method, clamp=[-1]).contiguous()      # [T, B, N]
        for k0 in range(0, G, k_max):
            batch = genes[k0:k0 + k_max]
            for j, this_gene in enumerate(batch):
                y0s[j].copy_(y0)
                y0s[j, :, 0, this_gene] = values[k0 + j]
            sol = _calls_block(odenet, y0s[:len(batch)], t, method=method, clamp=batch)      # [T, k*B, N]
            engine.knockout_effects(base, sol, batch, scores=scores[k0:k0 + len(batch)],
                                    shift=shift[k0:k0 + len(batch)] if want_matrices else None,
                                    magnitude=magnitude[k0:k0 + len(batch)] if want_matrices else None)
            del sol       # one output block alive at a time
    return KnockoutEffects(genes, scores.cpu().numpy(), shift, magnitude)


KnockoutPairs = collections.namedtuple("KnockoutPairs", ("pairs", "genes", "scores", "interaction_scores", "shift", "magnitude",
                                                        "interaction", "interaction_magnitude", "singles"))


def _knockout_pairs_args(N, genes, pairs, value, pairs_per_launch):
    """(genes [G], values [G], pairs [K] of (a, b) genes, ia [K], ib [K] indices into genes) of `knockout_pairs`, checked
    on the host before any launch"""
    if genes is None and pairs is None:
        raise ValueError("knockout_pairs: give `genes` (all their pairs) or `pairs`; all pairs of all %d genes are never "
                         "implied" % N)
    if pairs is not None:
        pairs = [tuple(engine.int_list("knockout_pairs", p, "the genes of a pair"))
                 for p in (pairs.tolist() if hasattr(pairs, "tolist") else pairs)]
        seen = set()
        for p in pairs:
            if len(p) != 2:
                raise ValueError("knockout_pairs: a pair is two genes, got %r" % (p,))
            if p[0] == p[1]:
                raise ValueError("knockout_pairs: the pair (%d, %d) holds one gene twice" % p)
            if frozenset(p) in seen:
                raise ValueError("knockout_pairs: the pair (%d, %d) is listed twice" % p)
            seen.add(frozenset(p))
        if not pairs:
            raise ValueError("knockout_pairs: no pair to hold")
    if genes is None:
        genes = sorted(set(g for p in pairs for g in p))
    else:
        genes = engine.int_list("knockout_pairs", genes)
        if len(set(genes)) != len(genes):
            raise ValueError("knockout_pairs: a gene is listed twice in `genes`")
        if len(genes) < 2:
            raise ValueError("knockout_pairs: a pair needs two genes, `genes` names %d" % len(genes))
    engine.check_genes("knockout_pairs", genes + [g for p in (pairs or []) for g in p], N)
    index = {g: i for i, g in enumerate(genes)}
    if pairs is None:
        pairs = [(genes[i], genes[j]) for i in range(len(genes)) for j in range(i + 1, len(genes))]
    for p in pairs:
        if p[0] not in index or p[1] not in index:
            raise ValueError("knockout_pairs: the pair (%d, %d) names a gene that `genes` does not" % p)
    values = engine.gene_values("knockout_pairs", value, len(genes))
    if isinstance(pairs_per_launch, bool) or not hasattr(pairs_per_launch, "__index__") or int(pairs_per_launch) < 1:
        raise ValueError("knockout_pairs: pairs_per_launch must be a positive integer")
    return genes, values, pairs, [index[p[0]] for p in pairs], [index[p[1]] for p in pairs]


def knockout_pairs(odenet, y0, genes=None, pairs=None, value=0.0, time_pts_to_project=None, method="dopri5",
                   pairs_per_launch=8, want_matrices=True, max_singles_bytes=4 << 30):
    """Combination knockout screen: what does the system do when TWO genes are held together, and is the joint effect
    more or less than the sum of the single ones (epistasis, synthetic lethality, combination targets)?
    genes: G >= 2 distinct genes, all G (G - 1) / 2 pairs of them; or pairs: an explicit list of (a, b), a != b, no pair
    twice in either order (`genes` is then their sorted union unless given, and must name every gene of a pair).  One of
    the two must be given.  value: a scalar or one level per gene of `genes`; y0, time_pts_to_project, method as in
    `knockout_effects`.
    The baseline is solved once, the G single-gene calls once (width-1 sets in the clamped launches; that block,
    4 T G B N bytes, stays alive -- beyond `max_singles_bytes` the call is refused), then per block of `pairs_per_launch`
    pairs one clamped launch (`odeint_calls(clamp=[(a, b), ...])`) and one pass of phx_knockout_epistasis; one pair
    block is alive at a time.
    Returns KnockoutPairs(pairs, genes, scores, interaction_scores, shift, magnitude, interaction,
    interaction_magnitude, singles): with d_x = x - baseline over the projected time points after the first and the B
    states and e = d_ab - (d_a + d_b), shift / magnitude [K, N] are the means of d_ab / |d_ab|, interaction /
    interaction_magnitude those of e / |e| (device tensors, or None), scores / interaction_scores [K] (float32 numpy) the
    means of magnitude / interaction_magnitude over the targets n other than a and b, and `singles` the KnockoutEffects
    of the G single screens.  An interaction is a second-order difference of four solves: on weakly coupled weights it
    sits at the solver's tolerance."""
    N = params_of(odenet)[0].shape[1]
    genes, values, pairs, ia, ib = _knockout_pairs_args(N, genes, pairs, value, pairs_per_launch)   # first, whatever else holds
    G, K = len(genes), len(pairs)

    def singles_fit(T, B):
        if 4 * T * G * B * N > max_singles_bytes:
            raise ValueError("knockout_pairs: the block of the %d single-gene solves takes 4 T G B N = %d bytes, more than "
                             "max_singles_bytes = %d; screen fewer genes at a time" % (G, 4 * T * G * B * N, max_singles_bytes))

    y0, t = _screen_setup("knockout_pairs", odenet, y0, time_pts_to_project, N, singles_fit)
    device, B = y0.device, y0.shape[0]
    k_max = max(1, min(int(pairs_per_launch), K))
    out = [torch.empty(K, dtype=torch.float32, device=device) for _ in range(2)]
    out += [torch.empty((K, N), dtype=torch.float32, device=device) if want_matrices else None for _ in range(4)]
    with torch.no_grad():
        base = _calls_block(odenet, y0.unsqueeze(0), t, method=method, clamp=[-1]).contiguous()      # [T, B, N]
        y0s = y0.unsqueeze(0).repeat(G, 1, 1, 1)
        for g in range(G):
            y0s[g, :, 0, genes[g]] = values[g]
        singles = _calls_block(odenet, y0s, t, method=method, clamp=genes).contiguous()              # [T, G*B, N]
        one = engine.knockout_effects(base, singles, genes, want_matrices=want_matrices)
        y0s = torch.empty((k_max, B, 1, N), dtype=torch.float32, device=device)
        for k0 in range(0, K, k_max):
            k1 = min(K, k0 + k_max)
            for j in range(k1 - k0):
                y0s[j].copy_(y0)
                y0s[j, :, 0, pairs[k0 + j][0]] = values[ia[k0 + j]]
                y0s[j, :, 0, pairs[k0 + j][1]] = values[ib[k0 + j]]
            sol = _calls_block(odenet, y0s[:k1 - k0], t, method=method, clamp=pairs[k0:k1])          # [T, k*B, N]
            engine.knockout_epistasis(base, singles, sol.contiguous(), ia[k0:k1], ib[k0:k1], genes,
                                      out=[None if x is None else x[k0:k1] for x in out])
            del sol       # one pair block alive at a time
    return KnockoutPairs(pairs, genes, out[0].cpu().numpy(), out[1].cpu().numpy(), out[2], out[3], out[4], out[5],
                         KnockoutEffects(genes, one[0].cpu().numpy(), one[1], one[2]))


def effects_matrix(odenet, rows=None, out=None):
    """The reference's regulatory "effects matrix" (extract_model_matrix_PHOENIX.py:46-58) on the device:
    effects[i, j] = relu(g_j) * (Ws^T Wa[:, :H]^T + Wp^T Wa[:, H:]^T)[i, j], regulator i -> target j, float32 [R, N].
    `rows = (row0, row1)` computes regulator rows row0 .. row1 - 1 only (R = row1 - row0): at genome scale the matrix is
    0.5 to 0.9 GB, and a caller may want it in pieces; `out` is written in place.  What the reference then dumps as CSV is
    `.cpu().numpy()` of the result."""
    tensors = params_of(odenet)
    rows = engine.check_rows(rows, tensors[0].shape[1])
    engine._require_gpu(tensors[0], "odenet")
    with torch.no_grad():
        return engine.effects_matrix(engine.params_cached(*tensors), "effects", rows=rows, out=out)


def jacobian_matrix(odenet, y, reduce="mean_abs", rows=None, out=None):
    """The Jacobian of the RHS (odenet.py:85-91) over a batch of expression states `y` ([B, N] or [B, 1, N], float32, on the
    device), J_b[i, j] = d f_j / d y_i at y_b, averaged over the batch as it is (reduce="mean") or in absolute value
    (reduce="mean_abs"): the state-dependent regulator -> target network that the influence scan samples by perturbation
    and of which `effects_matrix` is the crude, state-free form.  float32 [R, N] on the device; `rows` and `out` as for
    `effects_matrix`.  One kernel call: the [N, N] Jacobians of the states are never formed."""
    with torch.no_grad():
        p, mode, y2, ph, rows = _model_states(odenet, y, reduce, lambda N: engine.check_rows(rows, N), need_y=True)
        return engine.effects_matrix(p, mode, y=y2, ph=ph, rows=rows, out=out)


def _states(p, y):
    """(y [B, N] contiguous, ph [B, H]) of states `y` ([B, N] or [B, 1, N]) for the Jacobian modes of the engine"""
    N = p.N
    engine._require_gpu(y, "y")
    if not ((y.dim() == 2 and y.shape[1] == N) or (y.dim() == 3 and y.shape[1:] == (1, N))) or y.shape[0] < 1:
        raise ValueError("y must be [B, %d] or [B, 1, %d], got %s" % (N, N, tuple(y.shape)))
    y2 = y.detach().reshape(y.shape[0], N).contiguous()
    # the product branch's hidden vector of every state (odenet.py:87-88): a [B, N] x [N, H] contraction, plumbing
    s = y2 - 0.5
    return y2, torch.exp(torch.addmm(p.bp, torch.log1p(s / (1 + s.abs())), p.Wp.t()))


def _model_states(odenet, y, reduce, host_check=None, name=None, need_y=False):
    """What the analyses of the effects tile engine do before they call it, host errors first: the `reduce` check (its
    message starts with `name` where one is given), then host_check(N) -- the caller's ValueErrors that need the gene
    count -- and only then the requirement of a GPU.  Returns (Params, mode, y2, ph, what host_check returned): mode is
    "effects" and the states are None when `y` is None (never with `need_y`), else mode is `reduce`."""
    states = need_y or y is not None
    if states and reduce not in ("mean", "mean_abs"):
        raise ValueError('%sreduce must be "mean" or "mean_abs", got %r' % (name + ": " if name else "", reduce))
    tensors = params_of(odenet)
    checked = host_check(tensors[0].shape[1]) if host_check else None
    engine._require_gpu(tensors[0], "odenet")
    p = engine.params_cached(*tensors)
    y2, ph = _states(p, y) if states else (None, None)
    return p, reduce if states else "effects", y2, ph, checked


Edges = collections.namedtuple("Edges", ("regulator", "target", "value"))


def effects_edges(odenet, top=None, threshold=None, orient=False, diagonal=False, y=None, reduce="mean_abs", max_edges=None):
    """The strongest regulator -> target edges of `effects_matrix(odenet)` (y=None) or of `jacobian_matrix(odenet, y,
    reduce)` without the [N, N] matrix: Edges(regulator int64 [E], target int64 [E], value float32 [E]) on the device,
    sorted by |value| descending, then regulator, then target; every value has the bits of the matrix entry.
    An entry is eligible when it is finite and non-zero and off the diagonal (`diagonal=True` admits the diagonal);
    `orient=True` keeps of every gene pair the strictly stronger direction only, the reference's `make_mask`
    (extract_model_matrix_PHOENIX.py:29-37): the diagonal and both directions of an equally strong pair are dropped.
    Exactly one of `threshold` (all eligible entries with |value| >= threshold) and `top` (the K strongest; ties at the
    cut go to the smaller regulator, then target; fewer than K eligible: all of them) selects.
    The kernel recomputes the tiles in every pass (count, at most one refinement, emit), so with `y` each pass repeats the
    loop over the states; `threshold` with `max_edges` is one pass into a list of that capacity and raises RuntimeError,
    naming the true count, when more entries qualify."""
    with torch.no_grad():
        p, mode, y2, ph, _ = _model_states(odenet, y, reduce, lambda N: engine.check_edges_selection(top, threshold, max_edges))
        return Edges(*engine.effects_edges(p, mode, y=y2, ph=ph, top=top, threshold=threshold, orient=orient,
                                           diagonal=diagonal, max_edges=max_edges))


Neighbors = collections.namedtuple("Neighbors", ("gene", "value", "count", "strength"))


def effects_neighbors(odenet, k, of="target", regulators=None, targets=None, threshold=None, orient=False, diagonal=False,
                      y=None, reduce="mean_abs"):
    """Every gene's k strongest regulators (of="target": line j is column j of the matrix) or targets (of="regulator": line i
    is row i) in `effects_matrix(odenet)` (y=None) or `jacobian_matrix(odenet, y, reduce)`, without the [N, N] matrix:
    Neighbors(gene int64 [N, k], value float32 [N, k], count int64 [N], strength float32 [N]) on the device.  `gene` is the
    other gene's index, the entries of a line are sorted by |value| descending, then by that index; every value has the bits
    of the matrix entry; a line with fewer than k eligible entries is padded with gene = -1, value = +0.  `count` is the
    number of eligible entries of the line (with `threshold`: the in- or out-degree at that threshold), `strength` the
    float32 sum of their magnitudes (the weighted degree).
    Eligible are the entries `effects_edges` admits -- finite, non-zero, off the diagonal unless `diagonal=True`, with
    `orient=True` only the strictly stronger direction of a gene pair -- whose regulator is in `regulators` and whose target
    is in `targets` (sequences or tensors of gene indices, duplicates count once, None: all genes; e.g. a transcription-factor
    list, as get_link_list of GRN_rnaode.py:43-181 takes one) and, with `threshold` (positive, finite), |value| >= threshold.
    1 <= k <= 64.  One kernel call; the results are bitwise reproducible."""
    with torch.no_grad():
        p, mode, y2, ph, (k, _, regulators, targets) = _model_states(
            odenet, y, reduce, lambda N: engine.check_neighbors_selection(k, of, regulators, targets, threshold, N))
        return Neighbors(*engine.effects_neighbors(p, mode, k, of=of, y=y2, ph=ph, regulators=regulators, targets=targets,
                                                   threshold=threshold, orient=orient, diagonal=diagonal))


def effects_apply(odenet, v, of="target", weight="value", regulators=None, targets=None, threshold=None, orient=False,
                  diagonal=False, y=None, reduce="mean_abs"):
    """The product of a block of vectors `v` ([N] or [N, R], float32, on the device) with the inferred network, without the
    [N, N] matrix: with M = `effects_matrix(odenet)` (y=None) or `jacobian_matrix(odenet, y, reduce)`,
        of="target":     out[n, r] = sum_i w(M[i, n]) v[i, r]     scores flow regulator -> target, M^T v
        of="regulator":  out[n, r] = sum_j w(M[n, j]) v[j, r]     M v
    over the eligible entries only -- the rules of `effects_neighbors`: finite, non-zero, off the diagonal unless
    `diagonal=True`, with `orient=True` the strictly stronger direction of a gene pair, regulator in `regulators`, target in
    `targets`, |value| >= `threshold` -- with w the entry itself (weight="value"), its magnitude ("abs") or 1 ("unit").  The
    result has the shape of `v`, float32 on the device.  An ineligible entry is skipped, not multiplied by zero: a non-finite
    entry of M never reaches the result, and a non-finite v[g] reaches only the lines with an eligible entry at g; a line
    without eligible entries is +0.  Every sum has a fixed order: the result is bitwise reproducible, and a column's bits do
    not depend on the other columns of the block.  One kernel call per 32 columns."""
    with torch.no_grad():
        def host_check(N):
            checked = engine.check_apply_selection("effects_apply", of, weight, regulators, targets, threshold, N)
            engine.check_apply_block("effects_apply", v, N)
            return checked
        p, mode, y2, ph, (axis, wcode, regs, tgts) = _model_states(odenet, y, reduce, host_check)
        op = engine.ApplyOperator(p, mode, y=y2, ph=ph, regulators=regs, targets=tgts, threshold=threshold, orient=orient,
                                  diagonal=diagonal)
        return op.apply(v, axis, wcode)


Propagation = collections.namedtuple("Propagation", ("score", "iterations", "residual"))
PROPAGATION_DIRECTIONS = ("downstream", "upstream")
PROPAGATION_WEIGHTS = ("abs", "unit")


def propagation_steps(restart, tol):
    """the steps after which the walk is within `tol` of its fixed point in the 1-norm, from any start on the simplex: the
    map is a contraction with factor (1 - restart) and two distributions are at most 2 apart"""
    return max(1, int(np.ceil(np.log(tol / 2.0) / np.log1p(-restart))))


def _check_walk(name, N, seeds, restart, direction, weight, iterations, tol):
    """the ValueErrors of a propagation's own arguments; returns (p0 float64 numpy [N, R] with columns that sum to 1, whether
    the seeds were one-dimensional, the step count)"""
    if not isinstance(direction, str) or direction not in PROPAGATION_DIRECTIONS:
        raise ValueError('%s: direction must be "downstream" or "upstream", got %r' % (name, direction))
    if not isinstance(weight, str) or weight not in PROPAGATION_WEIGHTS:
        raise ValueError('%s: weight must be "abs" or "unit" (a walk has no signed weights), got %r' % (name, weight))
    number = (int, float, np.integer, np.floating)
    if not isinstance(restart, number) or isinstance(restart, bool) or not 0 < restart < 1:
        raise ValueError("%s: restart must lie strictly between 0 and 1, got %r" % (name, restart))
    if not isinstance(tol, number) or isinstance(tol, bool) or not 0 < tol < 2:
        raise ValueError("%s: tol must be positive (and below 2), got %r" % (name, tol))
    if iterations is not None and (not engine._is_int(iterations) or iterations < 1):
        raise ValueError("%s: iterations must be None or an integer >= 1, got %r" % (name, iterations))
    flat = True
    if seeds is None:
        p0 = np.full((N, 1), 1.0 / N)
    else:
        if isinstance(seeds, torch.Tensor):
            seeds = seeds.detach().cpu().numpy()
        try:
            s = np.asarray(seeds if hasattr(seeds, "shape") else list(seeds))
        except (TypeError, ValueError):
            raise ValueError("%s: seeds must be None, a sequence of gene indices or a tensor of weights" % name)
        if s.dtype == bool or s.dtype.kind not in "iuf":
            raise ValueError("%s: seeds must be gene indices or non-negative weights, got dtype %s" % (name, s.dtype))
        if s.dtype.kind in "iu" and s.ndim == 1 and not hasattr(seeds, "shape"):
            # a plain sequence of gene indices: every listed gene gets the same weight (duplicates count once)
            if s.size == 0 or s.min() < 0 or s.max() >= N:
                raise ValueError("%s: seeds must be gene indices in [0, %d), and at least one" % (name, N))
            p0 = np.zeros((N, 1))
            p0[s, 0] = 1.0
        else:
            if s.ndim not in (1, 2) or s.shape[0] != N or s.size == 0:
                raise ValueError("%s: seed weights must have the shape [%d] or [%d, R], got %s" % (name, N, N, s.shape))
            flat = s.ndim == 1
            p0 = s.reshape(N, -1).astype(np.float64)
            if not np.all(np.isfinite(p0)) or p0.min() < 0:
                raise ValueError("%s: seed weights must be finite and non-negative" % name)
        mass = p0.sum(axis=0)
        if np.any(mass <= 0):
            raise ValueError("%s: seed column %d has no mass" % (name, int(np.nonzero(mass <= 0)[0][0])))
        p0 = p0 / mass
    return p0, flat, propagation_steps(restart, tol) if iterations is None else int(iterations)


def _walk(apply, s, p0, restart, steps):
    """The random walk with restart, written once for the device and for `propagation_reference`: `steps` times
        p <- (1 - restart) (apply(p / s) + (mass of the genes with s = 0) p0) + restart p0
    from p = p0, with `apply` the weighted sum over the edges that end (or start) at each gene and s [N, 1] the genes'
    out- (or in-) strengths along the other axis, so that a gene hands its whole mass on, in proportion to the weights, and a
    gene without an edge hands it back to its walk's seeds.  p0, p [N, R]: tensors or arrays, whatever `apply` takes; nothing
    here reads a value on the host.  Returns (p, the 1-norm of the last step per column)."""
    live = s > 0
    dangling = 1.0 - live * 1.0
    inv = live / (s + dangling)                  # 1 / s, and 0 where s = 0
    p = p0
    step = p0 - p0
    for _ in range(steps):
        q = (1.0 - restart) * (apply(p * inv) + (p * dangling).sum(0) * p0) + restart * p0
        step, p = q - p, q
    return p, abs(step).sum(0)


def network_propagation(odenet, seeds=None, restart=0.5, direction="downstream", weight="abs", iterations=None, tol=1e-6,
                        regulators=None, targets=None, threshold=None, orient=False, diagonal=False, y=None,
                        reduce="mean_abs"):
    """Network propagation on the inferred network without the [N, N] matrix: a random walk with restart,
        p <- (1 - restart) W p + restart p0,
    along the eligible edges of `effects_apply` (same selection arguments), weighted by their magnitude (weight="abs") or all
    alike ("unit").  direction="downstream": a gene hands its mass to its targets, W[j, i] = w_ij / s_i with s_i = sum_j w_ij
    its out-strength; "upstream": to its regulators, the walk on the transposed network.  A gene without an outgoing edge
    hands its mass back to its walk's seeds.  `seeds`: None (uniform: with restart=0.15 this is PageRank on the network), a
    sequence of gene indices, or a [N] or [N, R] tensor of non-negative weights, one walk per column; columns are scaled to
    sum 1.  The map contracts the 1-norm by (1 - restart), so `iterations=None` takes ceil(log(tol / 2) / log(1 - restart))
    steps, after which every walk is within `tol` of its fixed point, without a host synchronisation inside the loop.
    Returns Propagation(score float32 [N] or [N, R] on the device, iterations, residual: the 1-norm of the last step per
    column, read once at the end)."""
    name = "network_propagation"
    with torch.no_grad():
        def host_check(N):
            walk = _check_walk(name, N, seeds, restart, direction, weight, iterations, tol)
            return engine.check_apply_selection(name, "target", weight, regulators, targets, threshold, N), walk
        p, mode, y2, ph, ((_, wcode, regs, tgts), (p0, flat, steps)) = _model_states(odenet, y, reduce, host_check, name=name)
        op = engine.ApplyOperator(p, mode, y=y2, ph=ph, regulators=regs, targets=tgts, threshold=threshold, orient=orient,
                                  diagonal=diagonal, name=name)
        along, across = ("target", "regulator") if direction == "downstream" else ("regulator", "target")
        p0 = torch.from_numpy(p0.astype(np.float32)).to(p.device)
        s = op.apply(torch.ones((p.N, 1), dtype=torch.float32, device=p.device), across, wcode)
        score, residual = _walk(lambda x: op.apply(x, along, wcode), s, p0, restart, steps)
        residual = residual.cpu().numpy()
        return Propagation(score[:, 0] if flat else score, steps, residual[0] if flat else residual)


def _eligible(M, regulators, targets, threshold, orient, diagonal):
    """the eligibility of `effects_neighbors` on a dense float32 matrix, as a boolean [N, N]"""
    N = M.shape[0]
    m = np.abs(M)
    ok = np.isfinite(m) & (m != 0)
    eye = np.eye(N, dtype=bool)
    if orient:
        with np.errstate(invalid="ignore"):
            ok &= ~eye & ~np.isnan(m.T) & (m > m.T)
    elif not diagonal:
        ok &= ~eye
    if regulators is not None:
        keep = np.zeros(N, bool)
        keep[np.asarray(list(regulators), np.int64)] = True
        ok &= keep[:, None]
    if targets is not None:
        keep = np.zeros(N, bool)
        keep[np.asarray(list(targets), np.int64)] = True
        ok &= keep[None, :]
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            ok &= m.astype(np.float64) >= float(threshold)
    return ok


def propagation_reference(matrix, seeds=None, restart=0.5, direction="downstream", weight="abs", iterations=None, tol=1e-6,
                          regulators=None, targets=None, threshold=None, orient=False, diagonal=False):
    """`network_propagation` on a dense regulator -> target matrix (float32 [N, N], e.g. what `effects_matrix` returned,
    brought to the host), in numpy float64 and without a GPU: the same walk (`_walk`), with the edge sums taken on the
    matrix.  Propagation(score float64 [N] or [N, R], iterations, residual)."""
    name = "propagation_reference"
    M = np.asarray(matrix)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 2:
        raise ValueError("%s: the matrix must be [N, N] with N >= 2, got %s" % (name, M.shape))
    N = M.shape[0]
    p0, flat, steps = _check_walk(name, N, seeds, restart, direction, weight, iterations, tol)
    _, _, regs, tgts = engine.check_apply_selection(name, "target", weight, regulators, targets, threshold, N)
    ok = _eligible(M.astype(np.float32), None if regs is None else regs.tolist(), None if tgts is None else tgts.tolist(),
                   threshold, orient, diagonal)
    W = np.zeros((N, N))
    W[ok] = 1.0 if weight == "unit" else np.abs(M[ok]).astype(np.float64)
    if direction == "downstream":                 # along the columns: the regulators' mass arrives at their targets
        s, apply = W.sum(axis=1)[:, None], lambda x: W.T @ x
    else:
        s, apply = W.sum(axis=0)[:, None], lambda x: W @ x
    score, residual = _walk(apply, s, p0, restart, steps)
    return Propagation(score[:, 0] if flat else score, steps, residual[0] if flat else residual)


def write_link_list(fp, edges, gene_names=None, signed=False, of=None):
    """Writes the reference's ranked link-list file (get_link_list, GRN_rnaode.py:140-163): one line "regulator<TAB>target<TAB>
    score" per link, the score as %.6f.  `edges`: an `Edges`, written in its order, or a `Neighbors` together with the `of` it
    was made with ("target" / "regulator"), written line by line in its own order without the padding entries.  `gene_names`
    (one per gene, in row order) names the genes; without it they are written as G<index + 1>, the reference's default.  The
    score is |value|, or the value itself with `signed=True`.  `fp`: a path or an open text file.  Returns the number of
    links written."""
    if isinstance(edges, Neighbors):
        if of not in ("target", "regulator"):
            raise ValueError('write_link_list: a Neighbors needs of="target" or of="regulator", got %r' % (of,))
        gene = np.asarray(edges.gene.cpu() if isinstance(edges.gene, torch.Tensor) else edges.gene).astype(np.int64)
        value = np.asarray(edges.value.cpu() if isinstance(edges.value, torch.Tensor) else edges.value)
        line = np.broadcast_to(np.arange(gene.shape[0], dtype=np.int64)[:, None], gene.shape)
        keep = gene >= 0
        other, line, value = gene[keep], line[keep], value[keep]
        regulator, target = (other, line) if of == "target" else (line, other)
    elif isinstance(edges, Edges):
        if of is not None:
            raise ValueError("write_link_list: `of` belongs to a Neighbors")
        regulator, target, value = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in edges)
    else:
        raise ValueError("write_link_list: `edges` must be an Edges or a Neighbors, got %s" % type(edges).__name__)
    if gene_names is not None:
        gene_names = [str(n) for n in gene_names]
        if len(value) and max(int(regulator.max()), int(target.max())) >= len(gene_names):
            raise ValueError("write_link_list: %d gene names do not cover gene index %d"
                             % (len(gene_names), max(int(regulator.max()), int(target.max()))))
    score = value.astype(np.float64) if signed else np.abs(value.astype(np.float64))
    lines = []
    for i, j, s in zip(regulator.tolist(), target.tolist(), score.tolist()):
        if gene_names is not None:
            lines.append("%s\t%s\t%.6f\n" % (gene_names[i], gene_names[j], s))
        else:
            lines.append("G%d\tG%d\t%.6f\n" % (i + 1, j + 1, s))
    if hasattr(fp, "write"):
        fp.write("".join(lines))
    else:
        with open(fp, "w") as f:
            f.write("".join(lines))
    return len(lines)


def read_network(fp, gene_names):
    """Host parser of the reference's edge files (breast_cancer_data/clean_data/validation_network.csv, the simulator's
    edge_properties_G*.csv): a header row, then the regulator's and the target's gene name in the first two columns, quoted
    or not; further columns are ignored.  `gene_names`: the names of the model's genes in row order, a list or the path of
    a one-column names file with a header row (desmedt_gene_names_*.csv, gene_names_*.csv).  Returns (regulator, target) as
    int64 numpy arrays: rows that name an unknown gene and duplicates are dropped, the order is ascending (regulator,
    target)."""
    import csv
    if isinstance(gene_names, (str, bytes)) or hasattr(gene_names, "__fspath__"):
        with open(gene_names, newline="") as f:
            gene_names = [row[0] for row in list(csv.reader(f))[1:] if row]
    index = {}
    for k, name in enumerate(gene_names):
        index.setdefault(str(name), k)
    pairs = set()
    with open(fp, newline="") as f:
        rows = csv.reader(f)
        next(rows, None)                       # the header
        for row in rows:
            if len(row) < 2:
                continue
            i, j = index.get(row[0]), index.get(row[1])
            if i is not None and j is not None:
                pairs.add((i, j))
    pairs = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    return pairs[:, 0].copy(), pairs[:, 1].copy()


NetworkScore = collections.namedtuple("NetworkScore", ("auroc", "average_precision", "n_positive", "n_negative", "threshold",
                                                       "tp", "fp"))


def _network_call(name, odenet, regulator, target, y, reduce):
    """the checks `effects_at` and `network_score` share, in the order host errors first: (Params, mode, y2, ph, regulator,
    target) with the index tensors on the model's device"""
    p, mode, y2, ph, (regulator, target) = _model_states(
        odenet, y, reduce, lambda N: engine.check_network_indices(name, regulator, target, N), name=name)
    return p, mode, y2, ph, regulator.to(p.device), target.to(p.device)


def effects_at(odenet, regulator, target, orient=False, y=None, reduce="mean_abs"):
    """The entries (regulator[e], target[e]) of `effects_matrix(odenet)` (y=None) or of `jacobian_matrix(odenet, y, reduce)`
    without the [N, N] matrix: float32 [E] on the device, in the caller's order (duplicates allowed), every value with the
    bits of the matrix entry.  `orient=True` reads the reference's `make_mask` form of the matrix
    (extract_model_matrix_PHOENIX.py:29-37) instead: the weaker or equally strong direction of a gene pair and the diagonal
    are +0.  Only the 64 x 64 tiles that hold a listed entry are computed."""
    with torch.no_grad():
        p, mode, y2, ph, r, t = _network_call("effects_at", odenet, regulator, target, y, reduce)
        return engine.effects_gather(p, mode, r, t, y=y2, ph=ph, orient=orient)


def network_score(odenet, regulator, target, orient=False, diagonal=False, y=None, reduce="mean_abs"):
    """How well the model's network recovers a known one (the network-recovery AUROC of the PHOENIX paper; the reference's
    COMPUTE_GRN_AUROC, GRN_rnaode.py:10-22, without its list of all N^2 edges): every entry of `effects_matrix(odenet)`
    (y=None) or `jacobian_matrix(odenet, y, reduce)` is scored by its magnitude, the pairs (regulator[e], target[e]) -- e.g.
    from `read_network` -- are the positives (duplicates count once), every other scored entry is a negative.  Scored are
    all off-diagonal entries (get_link_list, GRN_rnaode.py:119: "Auto-regulations do not appear"); `diagonal=True` adds the diagonal, and
    positives on an excluded diagonal are dropped.  `orient=True` scores the `make_mask` form of the matrix (of every gene
    pair only the strictly stronger direction keeps its magnitude, everything else scores 0).  Zeros are scored like any
    other value: ties.
    Returns NetworkScore(auroc, average_precision, n_positive, n_negative, threshold, tp, fp): `threshold` float32 [m], the
    distinct magnitudes of the positives, descending; `tp`, `fp` int64 [m] on the device, the positives and negatives with
    magnitude >= threshold[k] (the ROC and precision-recall points at the thresholds where they bend); auroc and
    average_precision are Python floats with the tie handling of sklearn's roc_auc_score and average_precision_score,
    computed from exact integer counts.  The matrix is never formed: one kernel pass reads the positives' values, a second
    counts every entry against them.
    ValueError: index arrays of unequal length or out of range, a bad `reduce`, labels of one class only ("Only one class
    present"), or a scored entry that is not finite (the count is named)."""
    with torch.no_grad():
        p, mode, y2, ph, r, t = _network_call("network_score", odenet, regulator, target, y, reduce)
        return NetworkScore(*engine.network_score(p, mode, r, t, y=y2, ph=ph, orient=orient, diagonal=diagonal))


# ------------------------------------------------------------------ recovery of the simulator's Jacobian
JacobianRecovery = collections.namedtuple("JacobianRecovery", ("n_edges", "sign_agreement", "pearson", "spearman", "slope",
                                                               "regulator", "target", "true", "learned"))


def _average_ranks(v):
    """ranks 1 .. n of a float64 vector, ties sharing the mean of their positions (scipy's rankdata, method "average")"""
    order = np.argsort(v, kind="stable")
    s = v[order]
    first = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))      # where a run of equal values begins
    size = np.diff(np.concatenate((first, [len(v)])))
    ranks = np.empty(len(v), np.float64)
    ranks[order] = np.repeat(first + (size + 1) / 2.0, size)
    return ranks


def _pearson(a, b):
    if len(a) < 2:
        return float("nan")
    da, db = a - a.mean(), b - b.mean()
    saa, sbb = float(da @ da), float(db @ db)
    if not (saa > 0 and sbb > 0):                          # a constant vector has no correlation
        return float("nan")
    return float(min(1.0, max(-1.0, (da @ db) / np.sqrt(saa * sbb))))


def recovery_scores(true, learned):
    """(sign_agreement, pearson, spearman, slope) of two equally long vectors, Python floats computed in float64 on the host:
    sign_agreement -- the share of the entries with true != 0 at which `learned` has the sign of `true` (a learned 0
    disagrees); pearson -- the Pearson correlation; spearman -- the Pearson correlation of the average ranks; slope -- the
    least-squares s of learned ~ s * true through the origin, sum(true * learned) / sum(true^2).  A statistic that is not
    defined is NaN: the correlations of fewer than 2 entries or with a constant vector, the sign agreement and the slope of
    a `true` that is 0 throughout (or empty)."""
    t, l = np.asarray(true, np.float64).reshape(-1), np.asarray(learned, np.float64).reshape(-1)
    if t.shape != l.shape:
        raise ValueError("recovery_scores: true and learned must have the same length, got %d and %d" % (len(t), len(l)))
    nz = t != 0
    sign = float(np.mean(np.sign(t[nz]) == np.sign(l[nz]))) if nz.any() else float("nan")
    tt = float(t @ t)
    slope = float((t @ l) / tt) if tt > 0 else float("nan")
    return sign, _pearson(t, l), _pearson(_average_ranks(t), _average_ranks(l)), slope


def jacobian_recovery(odenet, system, x, diagonal=False):
    """How well a model trained on in-silico data recovers the simulator's signed, quantitative regulatory effects: on every
    entry of `system.jacobian_pattern()` (a `HillSystem`; the entries off the diagonal, `diagonal=True` adds the decay terms)
    true = `system.jacobian(x, "mean")`, the simulator's d rate_target / d x_regulator averaged over the states x ([B, N] or
    [B, 1, N], float32, on the device), is held against learned = `effects_at(odenet, regulator, target, y=x, reduce="mean")`,
    the model's, with the bits of `jacobian_matrix(odenet, x, "mean")`.  Returns JacobianRecovery(n_edges, sign_agreement,
    pearson, spearman, slope, regulator, target, true, learned): the four statistics of `recovery_scores(true, learned)`,
    the entries as int64 [n_edges] and the two vectors as float32 [n_edges] on the device.  Where `network_score` asks
    whether the edges are found, this asks whether their signs and strengths are right.
    ValueError when the model's gene count is not `system.N`, or for an `x` of another shape."""
    tensors = params_of(odenet)
    if tensors[0].shape[1] != system.N:
        raise ValueError("jacobian_recovery: the model has %d genes, the system %d" % (tensors[0].shape[1], system.N))
    pat = system.jacobian_pattern()
    keep = np.flatnonzero(np.ones(len(pat.regulator), bool) if diagonal else pat.regulator != pat.target)
    learned = effects_at(odenet, pat.regulator[keep], pat.target[keep], y=x, reduce="mean")
    jac = system.jacobian(x, "mean")
    at = torch.from_numpy(keep).to(jac.value.device)
    true = jac.value[at]
    scores = recovery_scores(true.cpu().numpy(), learned.cpu().numpy())
    return JacobianRecovery(len(keep), *scores, jac.regulator[at], jac.target[at], true, learned)


# ------------------------------------------------------------------ recovery of the simulator's knockout screen
KnockoutRecoveryScores = collections.namedtuple("KnockoutRecoveryScores", ("n_entries", "sign_agreement", "pearson", "spearman",
                                                                           "slope", "per_gene"))
KnockoutPerGene = collections.namedtuple("KnockoutPerGene", ("n_entries", "sign_agreement", "pearson", "spearman", "slope"))
KnockoutRecovery = collections.namedtuple("KnockoutRecovery", ("genes", "n_entries", "sign_agreement", "pearson", "spearman",
                                                               "slope", "per_gene", "scores_spearman", "true", "learned"))


def knockout_recovery_scores(genes, true_shift, learned_shift, min_effect=0.0):
    """`recovery_scores` of two knockout screens' shift matrices ([G, N], tensors or arrays; float64 on the host).  Entry
    (i, n) counts iff n != genes[i] (the held gene itself is no prediction) and |true_shift[i, n]| > min_effect (with the
    default 0: the genes the held gene reaches at all -- the truth is exactly 0 elsewhere).  Returns
    KnockoutRecoveryScores(n_entries, sign_agreement, pearson, spearman, slope, per_gene): the four statistics pooled over
    the counted entries, and per_gene = KnockoutPerGene(n_entries int64 [G], sign_agreement, pearson, spearman, slope
    float64 [G]), the same over the counted entries of each knockout.  A statistic that is not defined is NaN, as there:
    every one of a knockout (or a screen) without a counted entry."""
    t, l = _host_array(true_shift).astype(np.float64), _host_array(learned_shift).astype(np.float64)
    genes = [int(g) for g in genes]
    if t.ndim != 2 or t.shape != l.shape or t.shape[0] != len(genes):
        raise ValueError("knockout_recovery_scores: true_shift and learned_shift must both be [%d, N], got %s and %s"
                         % (len(genes), t.shape, l.shape))
    G, N = t.shape
    for g in genes:
        if g < 0 or g >= N:
            raise ValueError("knockout_recovery_scores: gene %d is not one of 0 .. %d" % (g, N - 1))
    if not float(min_effect) >= 0:
        raise ValueError("knockout_recovery_scores: min_effect must be >= 0, got %r" % (min_effect,))
    counted = np.abs(t) > float(min_effect)
    counted[np.arange(G), genes] = False
    per = np.full((G, 4), np.nan)
    for i in range(G):
        per[i] = recovery_scores(t[i, counted[i]], l[i, counted[i]])
    n_each = counted.sum(axis=1).astype(np.int64)
    return KnockoutRecoveryScores(int(n_each.sum()), *recovery_scores(t[counted], l[counted]),
                                  KnockoutPerGene(n_each, per[:, 0].copy(), per[:, 1].copy(), per[:, 2].copy(), per[:, 3].copy()))


def knockout_recovery(odenet, system, y0, genes=None, value=0.0, time_pts_to_project=None, method="dopri5", dt_max=0.01,
                      min_effect=0.0, genes_per_launch=8):
    """Does a model trained on in-silico data predict what the simulator does under a knockout?  The model's screen,
    `knockout_effects(odenet, y0, genes, value, time_pts_to_project, method, genes_per_launch)`, is held against the truth,
    `system.knockout_effects` (a `HillSystem`: the same states, genes, levels and time points, integrated with sub-steps <=
    dt_max), by `knockout_recovery_scores` on the two shift matrices.  Returns KnockoutRecovery(genes, n_entries,
    sign_agreement, pearson, spearman, slope, per_gene, scores_spearman, true, learned): the pooled statistics and those of
    every knockout; scores_spearman, the Spearman correlation of the two per-gene score vectors -- does the model rank the
    influential genes as the truth does, which is what `pathway_permutation_test` feeds on; and the two KnockoutEffects.
    Where `jacobian_recovery` asks about local slopes, this asks about the response to a sustained intervention.
    ValueError before any launch when the model's gene count is not `system.N`."""
    N = params_of(odenet)[0].shape[1]
    if N != system.N:
        raise ValueError("knockout_recovery: the model has %d genes, the system %d" % (N, system.N))
    genes, values = _knockout_args(N, genes, value, genes_per_launch)
    if time_pts_to_project is None:
        time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))
    learned = knockout_effects(odenet, y0, genes, values, time_pts_to_project, method, genes_per_launch)
    true = system.knockout_effects(y0, genes, values, time_pts_to_project, dt_max)
    s = knockout_recovery_scores(genes, true.shift, learned.shift, min_effect)
    a, b = np.asarray(true.scores, np.float64), np.asarray(learned.scores, np.float64)
    return KnockoutRecovery(genes, s.n_entries, s.sign_agreement, s.pearson, s.spearman, s.slope, s.per_gene,
                            _pearson(_average_ranks(a), _average_ranks(b)), true, learned)


# ------------------------------------------------------------------ recovery of the simulator's pair screen (epistasis)
EpistasisRecoveryScores = collections.namedtuple("EpistasisRecoveryScores", ("n_entries", "sign_agreement", "pearson", "spearman",
                                                                             "slope", "per_pair"))
EpistasisPerPair = collections.namedtuple("EpistasisPerPair", ("n_entries", "sign_agreement", "pearson", "spearman", "slope"))
EpistasisRecovery = collections.namedtuple("EpistasisRecovery", ("pairs", "n_entries", "sign_agreement", "pearson", "spearman",
                                                                 "slope", "per_pair", "joint", "scores_spearman", "true",
                                                                 "learned"))


def epistasis_recovery_scores(pairs, true_interaction, learned_interaction, min_effect=0.0):
    """`recovery_scores` of two pair screens' interaction matrices ([K, N], tensors or arrays; float64 on the host), built
    like `knockout_recovery_scores`.  Entry (k, n) counts iff n is neither gene of pairs[k] (a held gene is no prediction)
    and |true_interaction[k, n]| > min_effect (with the default 0: the common descendants of both genes -- the simulator's
    interaction is exactly 0 elsewhere).  Returns EpistasisRecoveryScores(n_entries, sign_agreement, pearson, spearman,
    slope, per_pair): the four statistics pooled over the counted entries, and per_pair = EpistasisPerPair(n_entries int64
    [K], sign_agreement, pearson, spearman, slope float64 [K]), the same over the counted entries of each pair.  A statistic
    that is not defined is NaN: every one of a pair (or a screen) without a counted entry."""
    t, l = _host_array(true_interaction).astype(np.float64), _host_array(learned_interaction).astype(np.float64)
    pairs = [tuple(int(g) for g in p) for p in pairs]
    if t.ndim != 2 or t.shape != l.shape or t.shape[0] != len(pairs):
        raise ValueError("epistasis_recovery_scores: true_interaction and learned_interaction must both be [%d, N], got %s "
                         "and %s" % (len(pairs), t.shape, l.shape))
    K, N = t.shape
    for p in pairs:
        if len(p) != 2 or min(p) < 0 or max(p) >= N:
            raise ValueError("epistasis_recovery_scores: %r is not a pair of genes of 0 .. %d" % (p, N - 1))
    if not float(min_effect) >= 0:
        raise ValueError("epistasis_recovery_scores: min_effect must be >= 0, got %r" % (min_effect,))
    counted = np.abs(t) > float(min_effect)
    for k, p in enumerate(pairs):
        counted[k, list(p)] = False
    per = np.full((K, 4), np.nan)
    for k in range(K):
        per[k] = recovery_scores(t[k, counted[k]], l[k, counted[k]])
    n_each = counted.sum(axis=1).astype(np.int64)
    return EpistasisRecoveryScores(int(n_each.sum()), *recovery_scores(t[counted], l[counted]),
                                   EpistasisPerPair(n_each, per[:, 0].copy(), per[:, 1].copy(), per[:, 2].copy(),
                                                    per[:, 3].copy()))


def epistasis_recovery(odenet, system, y0, genes=None, pairs=None, value=0.0, time_pts_to_project=None, method="dopri5",
                       dt_max=0.01, min_effect=0.0, pairs_per_launch=8):
    """Does a model trained on in-silico data recover the LOGIC of the network -- where two knockouts together do more or
    less than the sum of each alone?  The model's pair screen, `knockout_pairs(odenet, y0, genes, pairs, value,
    time_pts_to_project, method, pairs_per_launch)`, is held against the truth, `system.knockout_pairs` (a `HillSystem`
    whose targets combine their regulators through AND / OR / NOT gates: the same states, pairs, levels and time points,
    integrated with sub-steps <= dt_max).  Returns EpistasisRecovery(pairs, n_entries, sign_agreement, pearson, spearman,
    slope, per_pair, joint, scores_spearman, true, learned): `epistasis_recovery_scores` of the two interaction matrices,
    pooled and per pair; joint, the same of the two shift matrices of the pairs (is the joint effect itself predicted);
    scores_spearman, the Spearman correlation of the two interaction_scores vectors (does the model rank the interacting
    pairs as the truth does); and the two KnockoutPairs.  `HillSystem.coregulator_pairs` names the pairs that meet in a gate.
    ValueError before any launch when the model's gene count is not `system.N`."""
    N = params_of(odenet)[0].shape[1]
    if N != system.N:
        raise ValueError("epistasis_recovery: the model has %d genes, the system %d" % (N, system.N))
    genes, values, pairs, _, _ = _knockout_pairs_args(N, genes, pairs, value, pairs_per_launch)
    if time_pts_to_project is None:
        time_pts_to_project = torch.from_numpy(np.arange(0, 1, 0.1))
    learned = knockout_pairs(odenet, y0, genes, pairs, values, time_pts_to_project, method, pairs_per_launch)
    true = system.knockout_pairs(y0, genes, pairs, values, time_pts_to_project, dt_max)
    s = epistasis_recovery_scores(pairs, true.interaction, learned.interaction, min_effect)
    joint = epistasis_recovery_scores(pairs, true.shift, learned.shift, min_effect)
    a, b = np.asarray(true.interaction_scores, np.float64), np.asarray(learned.interaction_scores, np.float64)
    return EpistasisRecovery(pairs, s.n_entries, s.sign_agreement, s.pearson, s.spearman, s.slope, s.per_pair, joint,
                             _pearson(_average_ranks(a), _average_ranks(b)), true, learned)


# ------------------------------------------------------------------ recovery of the simulator's attractors
SteadyStateRecovery = collections.namedtuple("SteadyStateRecovery", ("genes", "n_entries", "sign_agreement", "pearson", "spearman",
                                                                     "slope", "per_gene", "base_pearson", "base_rms",
                                                                     "scores_spearman", "n_unconverged", "true", "learned"))


def steady_state_recovery_scores(genes, true, learned, regulated=None, min_effect=0.0):
    """The statistics of `steady_state_recovery` from the two screens' results, on the host in float64.  true / learned:
    `KnockoutSteadyStates` (or anything with their fields; tensors or arrays) of the same K genes over the same B states.
    A row -- an unperturbed state b, or a knockout row k B + b -- counts iff its status is 0 on BOTH sides; shift and
    magnitude [K, N] are the means over the counted rows of each knockout (NaN for a knockout without one, which
    `knockout_recovery_scores` then leaves out: |NaN| > min_effect is false).  regulated: bool [N], the genes the states are
    compared on (default all).  Returns SteadyStateRecovery(genes, n_entries, sign_agreement, pearson, spearman, slope,
    per_gene -- `knockout_recovery_scores` of the two shift matrices --, base_pearson, base_rms -- the Pearson correlation
    and the root mean square distance of the two sets of unperturbed settled states over the counted rows and the regulated
    genes --, scores_spearman -- the Spearman correlation of the per-knockout means of the magnitude over the genes other
    than the held one --, n_unconverged -- the rows left out --, true, learned)."""
    genes = [int(g) for g in genes]
    K = len(genes)
    tb, lb = _host_array(true.base.y).astype(np.float64), _host_array(learned.base.y).astype(np.float64)
    tk, lk = _host_array(true.knockouts.y).astype(np.float64), _host_array(learned.knockouts.y).astype(np.float64)
    if tb.ndim != 2 or tb.shape != lb.shape or tk.shape != lk.shape or tk.shape != (K * tb.shape[0], tb.shape[1]):
        raise ValueError("steady_state_recovery_scores: the two screens must hold the same [B, N] states and [%d B, N] "
                         "knockout rows, got %s, %s and %s, %s" % (K, tb.shape, tk.shape, lb.shape, lk.shape))
    B, N = tb.shape
    regulated = np.ones(N, bool) if regulated is None else np.asarray(regulated, bool).reshape(-1)
    if regulated.shape != (N,):
        raise ValueError("steady_state_recovery_scores: regulated must be bool [%d]" % N)
    ok_b = (_host_array(true.base.status) == 0) & (_host_array(learned.base.status) == 0)
    ok_k = ((_host_array(true.knockouts.status) == 0) & (_host_array(learned.knockouts.status) == 0)).reshape(K, B)
    shifts = []
    for kb, base in ((tk, tb), (lk, lb)):
        d = kb.reshape(K, B, N) - base[None, :, :]
        w = (ok_k & ok_b[None, :]).astype(np.float64)[:, :, None]
        with np.errstate(invalid="ignore"):
            shifts.append(((d * w).sum(axis=1) / w.sum(axis=1), (np.abs(d) * w).sum(axis=1) / w.sum(axis=1)))
    s = knockout_recovery_scores(genes, shifts[0][0], shifts[1][0], min_effect)
    a, b = tb[ok_b][:, regulated].reshape(-1), lb[ok_b][:, regulated].reshape(-1)
    rms = float(np.sqrt(np.mean((a - b) ** 2))) if len(a) else float("nan")
    others = np.ones((K, N), bool)
    others[np.arange(K), genes] = False
    with np.errstate(invalid="ignore"):
        mean_mag = [np.where(others, m, 0.0).sum(axis=1) / others.sum(axis=1) for m in (shifts[0][1], shifts[1][1])]
    live = np.isfinite(mean_mag[0]) & np.isfinite(mean_mag[1])
    rank = _pearson(_average_ranks(mean_mag[0][live]), _average_ranks(mean_mag[1][live]))
    return SteadyStateRecovery(genes, s.n_entries, s.sign_agreement, s.pearson, s.spearman, s.slope, s.per_gene,
                               _pearson(a, b), rms, rank, int((~ok_b).sum() + (~ok_k).sum()), true, learned)


def steady_state_recovery(odenet, system, y0, genes, value=0.0, min_effect=0.0, **steady_kw):
    """Does a model trained on in-silico data settle where the simulator settles, with and without a gene held?  The model's
    `steady.knockout_steady_states(odenet, y0, genes, value)` is held against the truth, `system.knockout_steady_states` (a
    `HillSystem`: the same states, genes and levels), by `steady_state_recovery_scores` with the system's regulated genes;
    steady_kw: tol, max_iter, tau0 of both.  Where `knockout_recovery` asks about the first unit of time after an
    intervention, this asks about its final outcome.  Returns the SteadyStateRecovery of the two screens.
    ValueError before any launch when the model's gene count is not `system.N`."""
    from . import steady
    N = params_of(odenet)[0].shape[1]
    if N != system.N:
        raise ValueError("steady_state_recovery: the model has %d genes, the system %d" % (N, system.N))
    if set(steady_kw) - {"tol", "max_iter", "tau0"}:
        raise TypeError("steady_state_recovery: unexpected arguments %s" % sorted(set(steady_kw) - {"tol", "max_iter", "tau0"}))
    genes = engine.int_list("steady_state_recovery", genes)
    engine.check_genes("steady_state_recovery", genes, N)
    learned = steady.knockout_steady_states(odenet, y0, genes, value, **steady_kw)
    true = system.knockout_steady_states(y0, genes, value, **steady_kw)
    return steady_state_recovery_scores(genes, true, learned, ~system.is_input, min_effect)


# ------------------------------------------------------------------ pathway permutation tests
def consolidate_gene_scores(gene_names, scores):
    """One score per gene symbol from one score per array entry (create_permutation_test_files_aws.R:68-84).  An entry
    whose name holds "///" names several genes: it is split, the parts are trimmed, every part inherits the entry's
    score, and a (part, score) pair that repeats within the entry is dropped.  A name that then occurs more than once
    gets the mean of its scores.  The order is the first appearance among the single-name entries followed by the split
    ones, as the script's `rbind` leaves them.  Returns (names: list of str, scores: float64 numpy array)."""
    gene_names = [str(n) for n in gene_names]
    scores = np.asarray(scores.detach().cpu() if isinstance(scores, torch.Tensor) else scores, dtype=np.float64).reshape(-1)
    if len(gene_names) != scores.shape[0]:
        raise ValueError("consolidate_gene_scores: %d names for %d scores" % (len(gene_names), scores.shape[0]))
    rows = [(n, s) for n, s in zip(gene_names, scores.tolist()) if "///" not in n]
    seen = set()
    for n, s in zip(gene_names, scores.tolist()):
        if "///" in n:
            for part in n.split("///"):
                part = part.strip()
                if (n, part, s) not in seen:
                    seen.add((n, part, s))
                    rows.append((part, s))
    groups = {}
    for n, s in rows:
        groups.setdefault(n, []).append(s)
    names = list(groups)
    return names, np.array([sum(groups[n]) / len(groups[n]) for n in names], dtype=np.float64)


Pathways = collections.namedtuple("Pathways", ("names", "ptr", "idx", "kept"))


def read_pathways(fp, gene_names):
    """Host parser of the reference's wide pathway table (<analysis>_pathway_binary_wide.csv): a header row with a
    `pathway` column and one column per gene, then one row of 0 / 1 per pathway; of a pathway that occurs again the first
    row counts.  The genes of `gene_names` (unique names, e.g. from `consolidate_gene_scores`) that are columns of the
    table are kept, in the order of `gene_names` (create_permutation_test_files_aws.R:90-100): the test permutes the
    scores of these genes only.  Returns Pathways(names, ptr, idx, kept): the pathway names in file order, the members
    in CSR form (`ptr` int64 [P + 1], `idx` int32 [nnz], ascending positions in the kept genes) and `kept` int64, the
    kept genes as indices into `gene_names` -- `scores[kept]` are the scores the members index."""
    import csv
    gene_names = [str(n) for n in gene_names]
    if len(set(gene_names)) != len(gene_names):
        raise ValueError("read_pathways: gene_names must be unique (consolidate_gene_scores makes them so)")
    f = fp if hasattr(fp, "read") else open(fp, newline="")
    try:
        rows = csv.reader(f)
        header = next(rows, None)
        if header is None or "pathway" not in header:
            raise ValueError("read_pathways: the table has no `pathway` column")
        column = {}
        for c, name in enumerate(header):
            column.setdefault(name, c)
        pcol = column.pop("pathway")
        kept = [k for k, n in enumerate(gene_names) if n in column]
        cols = [column[gene_names[k]] for k in kept]
        names, members, known = [], [], set()
        for row in rows:
            if not row or row[pcol] in known:
                continue
            known.add(row[pcol])
            names.append(row[pcol])
            members.append(np.nonzero(np.array([float(row[c]) for c in cols], dtype=np.float64))[0].astype(np.int32))
    finally:
        if f is not fp:
            f.close()
    ptr = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([len(m) for m in members], out=ptr[1:])
    idx = np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32)
    return Pathways(names, ptr, idx, np.array(kept, dtype=np.int64))


def _host_array(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def check_pathways(name, ptr, idx, N):
    """the ValueErrors of a CSR pathway list on the host, before a device is needed: (ptr int64, idx int64) as numpy"""
    ptr, idx = np.asarray(ptr), np.asarray(idx)
    if ptr.ndim != 1 or idx.ndim != 1 or ptr.dtype.kind not in "iu" or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("%s: ptr and idx must be one-dimensional integer arrays" % name)
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    if ptr.shape[0] < 2:
        raise ValueError("%s: at least one pathway is needed (ptr has P + 1 entries)" % name)
    if ptr[0] != 0 or ptr[-1] != idx.shape[0] or np.any(np.diff(ptr) < 0):
        raise ValueError("%s: ptr must start at 0, not decrease and end at len(idx) = %d" % (name, idx.shape[0]))
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        raise ValueError("%s: idx must lie in [0, %d), got %d .. %d" % (name, N, idx.min(), idx.max()))
    owner = np.repeat(np.arange(ptr.shape[0] - 1, dtype=np.int64), np.diff(ptr))
    if np.unique(owner * N + idx).shape[0] != idx.shape[0]:
        raise ValueError("%s: a pathway lists a gene more than once" % name)
    return ptr, idx


class PermutationTest:
    """The result of `pathway_permutation_test`: the raw sums of the permutations [first, first + n_perm) of `seed` --
    `base` float64 [P], `count` int64 [P], `s1`, `s2` float64 [P] (include/phoenix_hip.h: phx_pathway_permutations), on
    the device -- and, as properties computed from them in float64, the columns of the reference's output file with
    R = n_perm: `mean` = base + s1 / R, `sd` = sqrt(max(0, (s2 - s1^2 / R) / (R - 1))), `z` = (base - mean) / sd where
    sd > 0 and 0 elsewhere, `p` = count / R."""

    def __init__(self, base, count, s1, s2, n_perm, first, seed):
        self.base, self.count, self.s1, self.s2 = base, count, s1, s2
        self.n_perm, self.first, self.seed = int(n_perm), int(first), int(seed)

    @property
    def mean(self):
        return self.base + self.s1 / self.n_perm

    @property
    def sd(self):
        if self.n_perm < 2:
            raise ValueError("PermutationTest: a standard deviation needs at least 2 permutations")
        R = self.n_perm
        return torch.sqrt(torch.clamp((self.s2 - self.s1 * self.s1 / R) / (R - 1), min=0.0))

    @property
    def z(self):
        sd = self.sd
        live = sd > 0
        return torch.where(live, (self.base - self.mean) / torch.where(live, sd, torch.ones_like(sd)), torch.zeros_like(sd))

    @property
    def p(self):
        return self.count.to(torch.float64) / self.n_perm

    @staticmethod
    def merge(a, b):
        """The result over both ranges of two results of one seed on the same scores and pathways whose permutation
        ranges are adjacent (one ends where the other starts): how a run is extended, and how shards of the permutations
        (`parallel.shard_range`) are combined.  `b` is moved to `a`'s device."""
        if a.seed != b.seed:
            raise ValueError("PermutationTest.merge: different seeds (%d, %d)" % (a.seed, b.seed))
        if b.first < a.first:
            a, b = b, a
        if a.first + a.n_perm != b.first:
            raise ValueError("PermutationTest.merge: the ranges [%d, %d) and [%d, %d) are not adjacent and disjoint"
                             % (a.first, a.first + a.n_perm, b.first, b.first + b.n_perm))
        dev = a.base.device
        if a.base.shape != b.base.shape or not torch.equal(a.base, b.base.to(dev)):
            raise ValueError("PermutationTest.merge: the two results are not of the same scores and pathways")
        return PermutationTest(a.base, a.count + b.count.to(dev), a.s1 + b.s1.to(dev), a.s2 + b.s2.to(dev),
                               a.n_perm + b.n_perm, a.first, a.seed)


def pathway_permutation_test(scores, pathways, n_perm=500, seed=0, first=0, device="cuda"):
    """The permutation test of create_permutation_test_files_aws.R on the device: for every pathway, the sum of its genes'
    scores against the same sum under `n_perm` permutations of the gene labels.  `scores`: one score per kept gene
    (`scores[pathways.kept]` of the consolidated scores), finite; `pathways`: a `Pathways`, or any (names, ptr, idx, ...)
    with the members in CSR form.  At most 16384 genes.  Returns a `PermutationTest` on `device`.
    The permutations are numbered: number r of `seed` is the same on every device and in every call, and this call takes
    [first, first + n_perm), so a run is extended or sharded by `first` and joined with `PermutationTest.merge`.  All
    pathways see the same permutation r; the reference draws a fresh one per pathway and replicate.  The null distribution of
    every single pathway is the same either way, only the dependence between the statistics of different pathways differs.
    first + n_perm >= 2 (a standard deviation needs two draws)."""
    name = "pathway_permutation_test"
    seed, first, n_perm = engine.check_permutation_range(name, seed, first, n_perm)
    if first + n_perm < 2:
        raise ValueError("%s: first + n_perm must be at least 2, got %d + %d" % (name, first, n_perm))
    s = scores.detach() if isinstance(scores, torch.Tensor) else _host_array(scores).astype(np.float32)
    if s.ndim != 1 or not 1 <= s.shape[0] <= 16384:
        raise ValueError("%s: scores must be [N] with 1 <= N <= 16384, got %s" % (name, tuple(s.shape)))
    ptr, idx = check_pathways(name, _host_array(pathways[1]), _host_array(pathways[2]), s.shape[0])
    if not isinstance(s, torch.Tensor):
        s = torch.from_numpy(np.ascontiguousarray(s))
    if not bool(torch.isfinite(s).all()):
        raise ValueError("%s: scores must be finite" % name)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("phoenix_amd: %s runs on the GPU (cuda/HIP device) only, got device %r" % (name, str(device)))
    with torch.no_grad(), torch.cuda.device(device):
        s = s.to(device=device, dtype=torch.float32)
        out = engine.pathway_permutations(s, torch.from_numpy(ptr).to(device), torch.from_numpy(idx.astype(np.int32)).to(device),
                                          seed, first, n_perm)
    return PermutationTest(*out, n_perm=n_perm, first=first, seed=seed)


def write_permutation_table(fp, result, pathway_names):
    """Writes the reference's output file (create_permutation_test_files_aws.R:114-116, `write.csv(..., row.names = F)`):
    the header "pathway","phnx_z_score","mean_path_score","sd_path_score","phnx_p_val", then one row per pathway sorted
    by z descending (stably: equal z keep the order of `pathway_names`), the name quoted, the numbers as %.15g.  `fp`: a
    path or an open text file.  Returns the number of rows."""
    names = [str(n) for n in pathway_names]
    cols = [np.asarray(x.detach().cpu(), dtype=np.float64) for x in (result.z, result.mean, result.sd, result.p)]
    if any(c.shape != (len(names),) for c in cols):
        raise ValueError("write_permutation_table: %d names for %d pathways" % (len(names), cols[0].shape[0]))
    lines = ['"pathway","phnx_z_score","mean_path_score","sd_path_score","phnx_p_val"\n']
    for k in np.argsort(-cols[0], kind="stable").tolist():
        lines.append('"%s",%.15g,%.15g,%.15g,%.15g\n' % ((names[k].replace('"', '""'),) + tuple(float(c[k]) for c in cols)))
    if hasattr(fp, "write"):
        fp.write("".join(lines))
    else:
        with open(fp, "w") as f:
            f.write("".join(lines))
    return len(names)
