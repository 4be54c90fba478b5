"""Row f4 of SURVEY.md section 8: the ground-truth Hill-kinetics simulator of the reference's in-silico data.

The reference generates its 350 / 690-gene training data in R: `GraphGRN_core.R:425-486` turns the regulatory graph
into one rate expression per gene (shipped as `ground_truth_simulator/clean_data/ode_system_functions_*.csv`, e.g.
`((1 * fAct(GAL11, 0.408, 1.797)) * 1 - 1 * A1_ALPHA2) / 1`; AND = product, OR = a + b - ab, NOT = 1 - a are already
spelled out in the text; `"input gene"` rows are held constant) and `SimulationGRN_core_init_var.R:203-247` draws
initial states and integrates every sample with `deSolve::ode`.  R is not available in this image, so this module
restates the simulator from those files: the expressions are compiled on the host into postfix programs and
evaluated / integrated on the GPU (`phx_hill_rhs`, `phx_hill_simulate` in `csrc/phx_hill.inc`), and the result is
written in the reference's CSV wire format (`csvreader.py:58-73`) so that `DataHandler.fromcsv` can train on it.
Parity: the RHS is checked against Python's own evaluation of the shipped expression strings (fp64) and the
trajectories against a tight-tolerance scipy solve of the same strings (golden G11); the R run itself cannot be
reproduced here (its RNG draws are not recorded), which DESIGN.md states.
The same programs are differentiated: `HillSystem.jacobian` (`phx_hill_jacobian`, `csrc/phx_hilljac.hip`) is the true
Jacobian of the rates on its sparse pattern, the ground truth `analysis.jacobian_recovery` scores a trained model against;
`jacobian_reference` restates it in numpy.
And perturbed: `HillSystem.knockouts` (`phx_hill_knockouts`, `csrc/phx_hillko.hip`) integrates the system with a gene held
at a level, `HillSystem.knockout_effects` scores such a screen as `analysis.knockout_effects` scores the model's -- the
ground truth of `analysis.knockout_recovery`; `rates_reference` / `knockouts_reference` restate them in numpy (section 8j).
A call may hold a SET of up to four genes (`phx_hill_knockout_sets`): `HillSystem.knockout_pairs` is the truth of
`analysis.knockout_pairs` and its epistasis score, `analysis.epistasis_recovery` scores a model against it (section 8l).
And where it settles: `HillSystem.steady_states` / `knockout_steady_states` (`phx_hill_steady`, `csrc/phx_hillss.hip`) relax
states to the system's attractors by the iteration of `steady.steady_states`, a step being a forward substitution over the
strongly connected components of the network (`block_structure`); `steady_states_reference` restates it in numpy, and
`analysis.steady_state_recovery` scores a model's settled states against it (section 8p).
"""
import ast
import collections
import csv
import ctypes as C

import numpy as np
import torch

from . import _lib, engine

OPS = {"PUSHC": 0, "PUSHX": 1, "ADD": 2, "SUB": 3, "MUL": 4, "DIV": 5, "NEG": 6, "FACT": 7}
MAX_STACK = 24   # HILL_STACK in csrc/phx_hill.inc


def fact_constants(ec50, n):
    """GraphGRN_core.R:431-434: B = (EC50^n - 1) / (2 EC50^n - 1), K_n = B - 1."""
    b = (ec50 ** n - 1.0) / (2.0 * ec50 ** n - 1.0)
    return b, b - 1.0, n


class _Compiler(ast.NodeVisitor):
    def __init__(self, index):
        self.index, self.code, self.consts, self.depth, self.max_depth = index, [], [], 0, 0

    def _push(self, op, arg=0):
        self.code.append((OPS[op], arg))
        self.depth += 1
        self.max_depth = max(self.max_depth, self.depth)

    def _const(self, *vals):
        k = len(self.consts)
        self.consts.extend(float(v) for v in vals)
        return k

    def visit_Expression(self, node):
        self.visit(node.body)

    def visit_Constant(self, node):
        self._push("PUSHC", self._const(node.value))

    def visit_Name(self, node):
        if node.id not in self.index:
            raise ValueError("unknown gene '%s' in a rate expression" % node.id)
        self._push("PUSHX", self.index[node.id])

    def visit_UnaryOp(self, node):
        self.visit(node.operand)
        if isinstance(node.op, ast.USub):
            self.code.append((OPS["NEG"], 0))
        elif not isinstance(node.op, ast.UAdd):
            raise ValueError("unsupported unary operator in a rate expression")

    def visit_BinOp(self, node):
        ops = {ast.Add: "ADD", ast.Sub: "SUB", ast.Mult: "MUL", ast.Div: "DIV"}
        if type(node.op) not in ops:
            raise ValueError("unsupported operator in a rate expression")
        self.visit(node.left)
        self.visit(node.right)
        self.code.append((OPS[ops[type(node.op)]], 0))
        self.depth -= 1

    def visit_Call(self, node):
        if not (isinstance(node.func, ast.Name) and node.func.id == "fAct" and len(node.args) == 3):
            raise ValueError("only fAct(TF, EC50, n) calls are supported in rate expressions")
        self.visit(node.args[0])
        ec50, n = (float(ast.literal_eval(a)) for a in node.args[1:])
        self.code.append((OPS["FACT"], self._const(*fact_constants(ec50, n))))

    def generic_visit(self, node):
        raise ValueError("unsupported syntax in a rate expression: %s" % type(node).__name__)


# ---------------------------------------------------------------------------------------------------------------------
# The equation builder (GraphGRN_core.R:163-190, 221-236, 312-330): how the reference turns a node's logic equation and the
# properties of its incoming edges into the rate-expression TEXT that it ships in ode_system_functions_*.csv.
#   NODE(tf)  ->  "<weight> * fAct(<tf>, <EC50>, <n>)"            (NODE: R:163-169, generateActivationEqnReg: R:312-330)
#   NOT(e)    ->  "(1 - e)"                                       (R:171-174)
#   AND(a, b) ->  "(a * b)"                                       (R:176-179)
#   OR(a, b)  ->  "(a + b - a * b)"                               (R:182-185)
#   rate      ->  "((act) * spmax - spdeg * NAME) / tau"          (generateRateEqn_modified: R:221-236)
# A logic tree is ("node", tf) | ("not", t) | ("and", a, b) | ("or", a, b).  The logic equations themselves are drawn at
# random when the reference builds its graph (genericLogicEqn, R:727-800: `runif(...) < propor`) and are NOT shipped, so
# they are recovered from the shipped expression text (`logic_of_expression`); what the pin (golden G16,
# tests/test_simulator_cpu.py) then checks is that `rate_expression(logic, edge properties)` reproduces every shipped
# expression text for text from edge_properties_G*.csv -- weights, EC50 and Hill constants as R printed them -- and that an
# edge is negated exactly where its `activation` flag is FALSE.
# ---------------------------------------------------------------------------------------------------------------------
def activation_text(edge):
    """`weight * fAct(from, EC50, n)` of one edge; `edge`: dict with the CSV's text fields from, weight, EC50, n"""
    return "%s * fAct(%s, %s, %s)" % (edge["weight"], edge["from"], edge["EC50"], edge["n"])


def logic_text(tree, node, edges):
    kind = tree[0]
    if kind == "node":
        return activation_text(edges[(tree[1], node)])
    if kind == "not":
        return "(1 - %s)" % logic_text(tree[1], node, edges)
    a, b = logic_text(tree[1], node, edges), logic_text(tree[2], node, edges)
    if kind == "and":
        return "(%s * %s)" % (a, b)
    if kind == "or":
        return "(%s + %s - %s * %s)" % (a, b, a, b)
    raise ValueError("unknown logic operator %r" % (kind,))


def rate_expression(node, tree, edges, spmax="1", spdeg="1", tau="1"):
    """generateRateEqn_modified (R:221-236) for a non-input node"""
    return "((%s) * %s - %s * %s) / %s" % (logic_text(tree, node, edges), spmax, spdeg, node, tau)


def logic_of_expression(expr, node):
    """inverse of `rate_expression`: (logic tree, spmax, spdeg, tau) recovered from a shipped expression string"""
    import re
    m = re.fullmatch(r"\(\((.*)\) \* (\S+) - (\S+) \* %s\) / (\S+)" % re.escape(node), expr)
    if not m:
        raise ValueError("not a rate expression of node %s: %s" % (node, expr[:80]))
    body, spmax, spdeg, tau = m.groups()
    pos = [0]

    def peek(txt):
        return body.startswith(txt, pos[0])

    def eat(txt):
        if not peek(txt):
            raise ValueError("expected %r at %d in %s" % (txt, pos[0], body[:120]))
        pos[0] += len(txt)

    def term():
        if peek("(1 - "):
            eat("(1 - ")
            t = term()
            eat(")")
            return ("not", t)
        if peek("("):
            eat("(")
            a = term()
            if peek(" * "):
                eat(" * ")
                b = term()
                eat(")")
                return ("and", a, b)
            eat(" + ")
            b = term()
            eat(" - ")
            a2 = term()
            eat(" * ")
            b2 = term()
            eat(")")
            if a2 != a or b2 != b:
                raise ValueError("malformed OR in %s" % body[:120])
            return ("or", a, b)
        m2 = re.compile(r"([0-9.eE+-]+) \* fAct\((\w+), ([0-9.eE+-]+), ([0-9.eE+-]+)\)").match(body, pos[0])
        if not m2:
            raise ValueError("expected an activation term at %d in %s" % (pos[0], body[:120]))
        pos[0] = m2.end()
        return ("node", m2.group(2), m2.group(1), m2.group(3), m2.group(4))

    t = term()
    if pos[0] != len(body):
        raise ValueError("trailing text in %s" % body[:120])

    def strip(x):   # leaves keep only the regulator's name: weight / EC50 / n come from the edge table when rebuilding
        return ("node", x[1]) if x[0] == "node" else (x[0],) + tuple(strip(y) for y in x[1:])

    def leaves(x, neg=False, out=None):
        out = [] if out is None else out
        if x[0] == "node":
            out.append((x[1], x[2], x[3], x[4], neg))
        elif x[0] == "not":
            leaves(x[1], not neg, out)
        else:
            for y in x[1:]:
                leaves(y, neg, out)
        return out

    return strip(t), spmax, spdeg, tau, leaves(t)


# ---------------------------------------------------------------------------------------------------------------------
# External inputs of a simulated data set (SimulationGRN_core_init_var.R:40-160).  Host-side sampling, as in the reference
# (R); the draws come from numpy's generator, so a data set is statistically, not bitwise, the reference's.
# ---------------------------------------------------------------------------------------------------------------------
def create_input_models(input_names, prop_bimodal=0.0, rng=None):
    """`createInputModels` (R:40-68): every input gene gets a one- or two-component normal mixture.
    Bimodal (probability `prop_bimodal`): weights (p, 1-p), p ~ U(0.2, 0.8); means Beta(10,100) and Beta(10,10).
    Unimodal: mean Beta(10,10).  sd = max(Beta(15,15) * min(mean, 1-mean)/3, 0.01) per component."""
    rng = np.random.default_rng() if rng is None else rng
    models = {}
    for name in input_names:
        if rng.random() < prop_bimodal:
            p = rng.uniform(0.2, 0.8)
            prop = np.array([p, 1.0 - p])
            mean = np.array([rng.beta(10, 100), rng.beta(10, 10)])
        else:
            prop = np.array([1.0])
            mean = np.array([rng.beta(10, 10)])
        maxsd = np.minimum(mean, 1.0 - mean) / 3.0
        sd = np.array([max(rng.beta(15, 15) * x, 0.01) for x in maxsd])
        models[name] = {"prop": prop, "mean": mean, "sd": sd}
    return models


def vine_correlation(d, betaparam=5.0, rng=None):
    """`vineS` (R:76-98): random correlation matrix by the C-vine construction of Lewandowski, Kurowicka and Joe (2009):
    partial correlations 2 Beta(b, b) - 1 (smaller `betaparam` = stronger correlations) converted to correlations, then a
    random simultaneous permutation of rows and columns.  The R loop starts at k = 2, so the first variable stays
    uncorrelated with the others before the permutation; kept.  d < 3: identity (the R loop bounds are not meaningful)."""
    rng = np.random.default_rng() if rng is None else rng
    S = np.eye(d)
    if d < 3:
        return S
    P = np.zeros((d, d))
    for k in range(1, d - 1):             # R: k in 2:(d-1), 1-based
        for i in range(k + 1, d):         # R: i in (k+1):d
            P[k, i] = (rng.beta(betaparam, betaparam) - 0.5) * 2.0
            p = P[k, i]
            for l in range(k - 1, -1, -1):    # R: l in (k-1):1
                p = p * np.sqrt((1.0 - P[l, i] ** 2) * (1.0 - P[l, k] ** 2)) + P[l, i] * P[l, k]
            S[k, i] = S[i, k] = p
    perm = rng.permutation(d)
    return S[np.ix_(perm, perm)]


def generate_input_data(models, numsamples, cor_strength=5.0, input_gene_var=1.0, rng=None):
    """`generateInputData` (R:101-160): [numsamples, n_inputs] external inputs in [0, 1] and the mixture classes.
    Every input is drawn from its mixture (component sd scaled by `input_gene_var`), out-of-range values are redrawn
    until none is left; with `cor_strength > 0` the unimodal inputs are then made rank-correlated: a multivariate normal
    sample with a `vine_correlation` matrix supplies the ranks, the sorted marginal draws supply the values (marginals
    unchanged); bimodal inputs keep their own draws ("avoid correlated bimodal inputs")."""
    rng = np.random.default_rng() if rng is None else rng
    names = list(models)
    X = np.full((numsamples, len(names)), -1.0)
    classf = {}
    for c, name in enumerate(names):
        m = models[name]
        mix = rng.choice(len(m["prop"]), size=numsamples, p=m["prop"])
        while True:
            out = (X[:, c] < 0) | (X[:, c] > 1)
            if not out.any():
                break
            for comp in range(len(m["prop"])):
                sel = out & (mix == comp)
                X[sel, c] = rng.normal(m["mean"][comp], m["sd"][comp] * input_gene_var, size=int(sel.sum()))
        if len(m["prop"]) > 1:
            classf[name] = mix + 1            # R's components are numbered from 1
    if cor_strength > 0 and numsamples > 1 and len(names) > 0:
        dm = np.sort(X, axis=0)
        cov = vine_correlation(len(names), cor_strength, rng)
        cordata = rng.multivariate_normal(np.zeros(len(names)), cov, size=numsamples, method="eigh")
        for c, name in enumerate(names):
            if name in classf:
                cordata[:, c] = X[:, c]
            else:
                ranks = np.argsort(np.argsort(cordata[:, c], kind="stable"), kind="stable")
                cordata[:, c] = dm[ranks, c]
        X = cordata
    return X, classf


def read_ode_system(path):
    """`ode_system_functions_*.csv`: columns node, eqn -> (names, expressions) in file order."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    return [r["node"] for r in rows], [r["eqn"] for r in rows]


HillPattern = collections.namedtuple("HillPattern", ("regulator", "target", "ptr"))
HillJacobian = collections.namedtuple("HillJacobian", ("regulator", "target", "value"))
HillBlocks = collections.namedtuple("HillBlocks", ("order", "comp_ptr", "level_ptr", "largest"))
SCC_MAX = 64     # PHX_HILL_SCC_MAX: the largest strongly connected component phx_hill_steady solves
JACOBIAN_MODES = {None: 0, "mean": 1, "mean_abs": 2}     # `mode` of phx_hill_jacobian
OP_HILL_JACOBIAN = 11    # workspace-cache key of HillSystem.jacobian (phx_hill_jacobian_workspace_bytes sizes it)


def _knockout_args(name, N, genes, value, lowest):
    """(genes, values) of a knockout screen of the simulator as lists of ints in lowest .. N - 1 and finite floats"""
    genes = list(range(N)) if genes is None else engine.int_list(name, genes)
    engine.check_genes(name, genes, N, lowest)
    if not genes:
        raise ValueError("%s: no gene to hold" % name)
    values = engine.gene_values(name, value, len(genes))
    for v in values:
        if not np.isfinite(np.float32(v)):
            raise ValueError("%s: level %r is not a finite float32" % (name, v))
    return genes, values


HOLD_MAX = 4     # PHX_HILL_HOLD_MAX: the genes one call of phx_hill_knockout_sets can hold


def _entries(xs):
    """a sequence or an array as a list whose array entries are lists"""
    xs = xs.tolist() if hasattr(xs, "tolist") else xs
    return [x.tolist() if hasattr(x, "tolist") else x for x in (xs if isinstance(xs, (list, tuple, range)) else [xs])]


def _names_sets(genes):
    """does `genes` of a knockout screen name a set anywhere (a sequence entry), or plain ints throughout"""
    return genes is not None and any(isinstance(e, (list, tuple, range)) for e in _entries(genes))


def _knockout_set_args(name, N, genes, value):
    """(sets, levels) of a knockout screen with held sets: per call the tuple of its distinct genes in 0 .. N - 1, in the
    order given (-1 entries dropped), and the tuple of their finite levels.  An entry of `genes` is an int or a sequence of
    at most HOLD_MAX ints; `value` a scalar, or per call a scalar or a sequence as long as that call's entry"""
    entries = _entries(genes)
    if not entries:
        raise ValueError("%s: no gene to hold" % name)
    values = _entries(value) if hasattr(value, "tolist") or isinstance(value, (list, tuple)) else [value] * len(entries)
    if len(values) != len(entries):
        raise ValueError("%s: %d values for %d calls" % (name, len(values), len(entries)))
    sets, levels = [], []
    for k, (entry, level) in enumerate(zip(entries, values)):
        held = engine.int_list(name, entry if isinstance(entry, (list, tuple, range)) else [entry])
        engine.check_genes(name, held, N, -1)
        if len(held) > HOLD_MAX:
            raise ValueError("%s: call %d names %d entries, a call holds at most %d genes" % (name, k, len(held), HOLD_MAX))
        if isinstance(level, (list, tuple)):
            if len(level) != len(held):
                raise ValueError("%s: call %d has %d levels for %d entries" % (name, k, len(level), len(held)))
        else:
            level = [level] * len(held)
        live = [(g, float(v)) for g, v in zip(held, level) if g >= 0]
        if len(set(g for g, _ in live)) != len(live):
            raise ValueError("%s: call %d names a gene twice: %r" % (name, k, tuple(held)))
        for _, v in live:
            if not np.isfinite(np.float32(v)):
                raise ValueError("%s: level %r is not a finite float32" % (name, v))
        sets.append(tuple(g for g, _ in live))
        levels.append(tuple(v for _, v in live))
    return sets, levels


def _knockout_times(name, times, dt_max):
    t64 = np.ascontiguousarray(_host_times(times), np.float64).reshape(-1)
    if t64.size < 1:
        raise ValueError("%s: no time point" % name)
    dt_max = float(dt_max)
    if not dt_max > 0:
        raise ValueError("%s: dt_max must be positive, got %r" % (name, dt_max))
    return t64, dt_max


def _host_times(times):
    return times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else np.asarray(times, np.float64)


class HillSystem:
    """The compiled rate expressions of one regulatory network, resident on the device."""

    def __init__(self, names, expressions, device="cuda"):
        self.names, self.expressions = list(names), list(expressions)
        self.N = len(self.names)
        index = {n: i for i, n in enumerate(self.names)}
        code, consts, off, length = [], [], [], []
        self.is_input = np.zeros(self.N, bool)
        for g, expr in enumerate(self.expressions):
            off.append(len(code))
            if expr.strip() == "input gene":            # GraphGRN_core.R:477-479
                self.is_input[g] = True
                length.append(0)
                continue
            c = _Compiler(index)
            c.visit(ast.parse(expr, mode="eval"))
            if c.max_depth > MAX_STACK:
                raise ValueError("rate expression of %s needs a deeper evaluation stack (%d)" % (self.names[g], c.max_depth))
            base = len(consts)
            code.extend((op, arg + base if op in (OPS["PUSHC"], OPS["FACT"]) else arg) for op, arg in c.code)
            consts.extend(c.consts)
            length.append(len(c.code))
        self.code_host = np.asarray(code, np.int32).reshape(-1, 2)
        self.consts_host = np.asarray(consts, np.float64)
        self.off_host, self.len_host = np.asarray(off, np.int32), np.asarray(length, np.int32)
        self._pattern = self._pattern_dev = self._blocks = self._blocks_dev = self._targets_of = None
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.code = torch.from_numpy(self.code_host).to(self.device)
            self.consts = torch.from_numpy(self.consts_host.astype(np.float32)).to(self.device)
            self.off = torch.from_numpy(self.off_host).to(self.device)
            self.len = torch.from_numpy(self.len_host).to(self.device)

    @classmethod
    def from_csv(cls, path, device="cuda"):
        return cls(*read_ode_system(path), device=device)

    # ---- device
    def _args(self):
        p = engine._p
        return p(self.code), p(self.off), p(self.len), p(self.consts)

    def rhs(self, x):
        """rates [B,N] at states x [B,N] (what `my_ode` returns, GraphGRN_core.R:441-470)."""
        engine._require_gpu(x, "x")
        x2 = x.detach().reshape(-1, self.N).contiguous().float()
        out = torch.empty_like(x2)
        engine._check_call(_lib.load().phx_hill_rhs(*self._args(), engine._p(x2), engine._p(out), x2.shape[0], self.N,
                                                    engine._stream_ptr()))
        return out.reshape(x.shape)

    def simulate(self, x0, times, dt_max=0.01):
        """states [T,B,N] at `times` (first row = x0), SimulationGRN_core_init_var.R:226-229,243-244."""
        engine._require_gpu(x0, "x0")
        x2 = x0.detach().reshape(-1, self.N).contiguous().float()
        t64 = torch.as_tensor(np.asarray(times, np.float64), device=x2.device)
        out = torch.empty((t64.numel(), x2.shape[0], self.N), dtype=torch.float32, device=x2.device)
        engine._check_call(_lib.load().phx_hill_simulate(*self._args(), engine._p(x2), engine._p(t64), t64.numel(),
                                                         C.c_double(dt_max), engine._p(out), x2.shape[0], self.N,
                                                         engine._stream_ptr()))
        return out

    # ---- knockout screens
    def _knockout_x0(self, name, x0, host_check=None):
        """x0 of a knockout screen as a contiguous float32 [B, N] tensor on the system's device; host_check(B): the caller's
        ValueErrors that need B, raised before a device is asked for"""
        N = self.N
        if not isinstance(x0, torch.Tensor):
            raise TypeError("%s: x0 must be a tensor on the GPU, got %s" % (name, type(x0).__name__))
        if (x0.dtype != torch.float32 or x0.shape[0] < 1 or
                not ((x0.dim() == 2 and x0.shape[1] == N) or (x0.dim() == 3 and x0.shape[1:] == (1, N)))):
            raise ValueError("%s: x0 must be float32 [B, %d] or [B, 1, %d], got %s %s" % (name, N, N, x0.dtype, tuple(x0.shape)))
        if host_check is not None:
            host_check(x0.shape[0])
        engine._require_gpu(x0, "x0")
        if self.device.type != "cuda" or x0.device != self.code.device:
            raise ValueError("%s: x0 is on %s, the system on %s" % (name, x0.device, self.device))
        return x0.detach().reshape(x0.shape[0], N).contiguous()

    def _knockouts(self, x2, t64, genes, values, dt_max):
        """phx_hill_knockouts on checked arguments: x2 [B, N], t64 [T] float64 on the device -> [T, K * B, N]"""
        K, B = len(genes), x2.shape[0]
        out = torch.empty((t64.numel(), K * B, self.N), dtype=torch.float32, device=x2.device)
        engine._check_call(_lib.load().phx_hill_knockouts(*self._args(), engine._p(x2), engine._p(t64), t64.numel(),
                                                          C.c_double(dt_max), (C.c_int * K)(*genes), (C.c_float * K)(*values), K,
                                                          engine._p(out), B, self.N, engine._stream_ptr()))
        return out

    def _knockout_sets(self, x2, t64, sets, levels, dt_max):
        """phx_hill_knockout_sets on checked arguments (`_knockout_set_args`): the rows padded with -1 to the widest set"""
        K, B, width = len(sets), x2.shape[0], max(1, max(len(s) for s in sets))
        genes = [g for s in sets for g in s + (-1,) * (width - len(s))]
        values = [v for l in levels for v in l + (0.0,) * (width - len(l))]
        out = torch.empty((t64.numel(), K * B, self.N), dtype=torch.float32, device=x2.device)
        engine._check_call(_lib.load().phx_hill_knockout_sets(*self._args(), engine._p(x2), engine._p(t64), t64.numel(),
                                                              C.c_double(dt_max), (C.c_int * (K * width))(*genes),
                                                              (C.c_float * (K * width))(*values), width, K, engine._p(out), B,
                                                              self.N, engine._stream_ptr()))
        return out

    def knockouts(self, x0, times, genes, value=0.0, dt_max=0.01):
        """`simulate` with a gene HELD at a level: states [T, K, B, N] float32 on the device, [:, k] the time course of the
        system started from x0 ([B, N] or [B, 1, N], float32, on the device) with column genes[k] set to value[k] and kept
        there -- its rate is 0 in every stage of every step, whatever its expression says (an "input gene" with that level).
        genes: K ints in -1 .. N - 1, -1 the unperturbed system; value: a scalar or [K] finite levels, 0 a knockout, a high
        level an over-expression.  The K calls share x0 (it is not replicated) and run in one pass (phx_hill_knockouts,
        include/phoenix_hip.h): `simulate`'s integrator, several calls of a sample per workgroup.  A call's bits do not depend
        on the calls beside it, so a gene that genes[k] does not reach (`jacobian_pattern`) equals the -1 call exactly.
        An entry of `genes` may also be a SET, a sequence of up to 4 distinct genes held together (`()` like -1: none; the
        shape `odeint_calls(clamp=...)` accepts); value[k] is then one level for all genes of call k or a sequence matching
        its entry.  A list with a set in it runs through phx_hill_knockout_sets, a list of plain ints as before; a call has
        the same bits either way, in either order of its set, whatever sets stand beside it.
        Argument errors are raised on the host before any launch."""
        sets = _names_sets(genes)
        genes, values = (_knockout_set_args("knockouts", self.N, genes, value) if sets else
                         _knockout_args("knockouts", self.N, genes, value, lowest=-1))
        t64, dt_max = _knockout_times("knockouts", times, dt_max)
        x2 = self._knockout_x0("knockouts", x0)
        out = (self._knockout_sets if sets else self._knockouts)(x2, torch.from_numpy(t64).to(x2.device), genes, values, dt_max)
        return out.reshape(len(t64), len(genes), x2.shape[0], self.N)

    def knockout_effects(self, x0, genes=None, value=0.0, times=None, dt_max=0.01, genes_per_launch=64, want_matrices=True):
        """The knockout screen of `analysis.knockout_effects` on the simulator itself -- the truth of that screen for a model
        trained on this system's data.  x0 [B, N] or [B, 1, N]: the states to start from; genes: the G genes to hold, one at
        a time (default: all N); value: a scalar or [G] levels; times: default the model screen's arange(0, 1, 0.1).
        The unperturbed system is a -1 call of `knockouts`; per block of `genes_per_launch` genes one `knockouts` pass and
        one pass of phx_knockout_effects against that baseline; one output block is alive at a time.
        Returns KnockoutEffects(genes, scores [G] float32 numpy, shift [G, N], magnitude [G, N] device tensors or None) with
        the meaning they have there: over the times after the first and the B states, shift[i, n] is the mean of held -
        baseline of gene n, magnitude[i, n] of its absolute value, scores[i] the mean of magnitude[i, n] over n != genes[i].
        Both are exactly 0 at a gene that genes[i] does not reach."""
        from .analysis import KnockoutEffects
        N = self.N
        genes, values = _knockout_args("knockout_effects", N, genes, value, lowest=0)
        if isinstance(genes_per_launch, bool) or not hasattr(genes_per_launch, "__index__") or int(genes_per_launch) < 1:
            raise ValueError("knockout_effects: genes_per_launch must be a positive integer")
        t64, dt_max = _knockout_times("knockout_effects", np.arange(0, 1, 0.1) if times is None else times, dt_max)
        if len(t64) < 2 or N < 2:
            raise ValueError("knockout_effects: needs at least two time points and two genes")
        x2 = self._knockout_x0("knockout_effects", x0)
        device, B, G, T = x2.device, x2.shape[0], len(genes), len(t64)
        k_max = min(int(genes_per_launch), G)
        t_dev = torch.from_numpy(t64).to(device)
        scores = torch.empty(G, dtype=torch.float32, device=device)
        shift = torch.empty((G, N), dtype=torch.float32, device=device) if want_matrices else None
        magnitude = torch.empty((G, N), dtype=torch.float32, device=device) if want_matrices else None
        base = self._knockouts(x2, t_dev, [-1], [0.0], dt_max)                     # [T, B, N]
        for k0 in range(0, G, k_max):
            batch = genes[k0:k0 + k_max]
            sol = self._knockouts(x2, t_dev, batch, values[k0:k0 + k_max], dt_max)     # [T, k * B, N]
            engine.knockout_effects(base, sol, batch, scores=scores[k0:k0 + len(batch)],
                                    shift=shift[k0:k0 + len(batch)] if want_matrices else None,
                                    magnitude=magnitude[k0:k0 + len(batch)] if want_matrices else None)
            del sol       # one output block alive at a time
        return KnockoutEffects(genes, scores.cpu().numpy(), shift, magnitude)

    def coregulator_pairs(self, genes=None):
        """The pairs that meet in a gate, on the host from `jacobian_pattern()`: the sorted list of (a, b), a < b, such that
        the program of some third gene j (not a, not b) reads both -- where a joint knockout can be non-additive at first
        order.  genes: only the pairs within that set of genes."""
        pat = self.jacobian_pattern()
        only = None if genes is None else set(engine.int_list("coregulator_pairs", genes))
        if only is not None:
            engine.check_genes("coregulator_pairs", sorted(only), self.N)
        pairs = set()
        for j in range(self.N):
            regs = [r for r in pat.regulator[pat.ptr[j]:pat.ptr[j + 1]].tolist() if r != j and (only is None or r in only)]
            pairs.update((a, b) for i, a in enumerate(regs) for b in regs[i + 1:])      # a row of the pattern ascends
        return sorted(pairs)

    def knockout_pairs(self, x0, genes=None, pairs=None, value=0.0, times=None, dt_max=0.01, pairs_per_launch=64,
                       want_matrices=True, max_singles_bytes=4 << 30):
        """The combination screen of `analysis.knockout_pairs` on the simulator itself -- the truth of that screen's epistasis
        for a model trained on this system's data; the targets here combine their regulators through AND / OR / NOT gates, so
        joint knockouts are non-additive.  genes / pairs / value / max_singles_bytes: the rules of `analysis.knockout_pairs`
        (G >= 2 distinct genes and all their pairs, or explicit pairs; a scalar or one level per gene); x0, times, dt_max as
        in `knockout_effects`.  The baseline is one -1 call and the G single-gene calls run once (phx_hill_knockouts; that
        block stays alive); per block of `pairs_per_launch` pairs one pass of phx_hill_knockout_sets and one of
        phx_knockout_epistasis; one pair block is alive at a time.
        Returns the KnockoutPairs of that screen, with the meaning its fields have there.  A call's bits do not depend on
        the calls beside it or on the width of its set, so interaction and interaction_magnitude are exactly 0 at every
        target that is not a common descendant of both genes of a pair: where a's knockout does not reach, the pair call
        has the bits of b's single call and a's single call those of the baseline."""
        from .analysis import KnockoutEffects, KnockoutPairs, _knockout_pairs_args
        N = self.N
        genes, values, pairs, ia, ib = _knockout_pairs_args(N, genes, pairs, value, pairs_per_launch)
        for v in values:
            if not np.isfinite(np.float32(v)):
                raise ValueError("knockout_pairs: level %r is not a finite float32" % v)
        t64, dt_max = _knockout_times("knockout_pairs", np.arange(0, 1, 0.1) if times is None else times, dt_max)
        if len(t64) < 2 or N < 3:
            raise ValueError("knockout_pairs: needs at least two time points and three genes")
        G, K, T = len(genes), len(pairs), len(t64)

        def singles_fit(B):
            if 4 * T * G * B * N > max_singles_bytes:
                raise ValueError("knockout_pairs: the block of the %d single-gene solves takes 4 T G B N = %d bytes, more than "
                                 "max_singles_bytes = %d; screen fewer genes at a time" % (G, 4 * T * G * B * N, max_singles_bytes))

        x2 = self._knockout_x0("knockout_pairs", x0, singles_fit)
        device = x2.device
        k_max = min(int(pairs_per_launch), K)
        t_dev = torch.from_numpy(t64).to(device)
        out = [torch.empty(K, dtype=torch.float32, device=device) for _ in range(2)]
        out += [torch.empty((K, N), dtype=torch.float32, device=device) if want_matrices else None for _ in range(4)]
        base = self._knockouts(x2, t_dev, [-1], [0.0], dt_max)                     # [T, B, N]
        singles = self._knockouts(x2, t_dev, genes, values, dt_max)                # [T, G * B, N]
        one = engine.knockout_effects(base, singles, genes, want_matrices=want_matrices)
        for k0 in range(0, K, k_max):
            k1 = min(K, k0 + k_max)
            sol = self._knockout_sets(x2, t_dev, pairs[k0:k1], [(values[ia[k]], values[ib[k]]) for k in range(k0, k1)], dt_max)
            engine.knockout_epistasis(base, singles, sol, ia[k0:k1], ib[k0:k1], genes,
                                      out=[None if x is None else x[k0:k1] for x in out])
            del sol       # one pair block alive at a time
        return KnockoutPairs(pairs, genes, out[0].cpu().numpy(), out[1].cpu().numpy(), out[2], out[3], out[4], out[5],
                             KnockoutEffects(genes, one[0].cpu().numpy(), one[1], one[2]))

    # ---- the true Jacobian
    def jacobian_pattern(self):
        """The sparsity pattern of the Jacobian of the rates, on the host: HillPattern(regulator int64 [E], target int64
        [E], ptr int64 [N + 1]) in CSR form by target -- regulator[ptr[j]:ptr[j + 1]] are the distinct genes the program of
        gene j pushes, ascending: its regulators and, through the decay term, itself.  "input gene" rows have no entries."""
        if self._pattern is None:
            pushx = self.code_host[:, 0] == OPS["PUSHX"]
            rows = [np.unique(self.code_host[o:o + n, 1][pushx[o:o + n]]) for o, n in zip(self.off_host, self.len_host)]
            ptr = np.zeros(self.N + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=ptr[1:])
            regulator = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
            target = np.repeat(np.arange(self.N, dtype=np.int64), np.diff(ptr))
            self._pattern = HillPattern(regulator, target, ptr)
        return self._pattern

    def _pattern_on_device(self):
        """(eptr int64 [N + 1], ereg int32 [E], regulator int64 [E], target int64 [E]) of the pattern on the system's device"""
        if self._pattern_dev is None:
            pat = self.jacobian_pattern()
            dev = self.code.device
            self._pattern_dev = (torch.from_numpy(pat.ptr).to(dev), torch.from_numpy(pat.regulator.astype(np.int32)).to(dev),
                                 torch.from_numpy(pat.regulator).to(dev), torch.from_numpy(pat.target).to(dev))
        return self._pattern_dev

    def jacobian(self, x, reduce=None):
        """The true Jacobian of the rates on `jacobian_pattern()`: HillJacobian(regulator int64 [E], target int64 [E], value
        float32) on the device, value[b, e] = d rate_target[e] / d x_regulator[e] at the state x[b] -- [B, E] with
        reduce=None, [E] with reduce="mean" (the mean over the states) or "mean_abs" (of the absolute value; both summed in
        float64 in an order that depends on B alone and rounded once).  x: [B, N] or [B, 1, N], float32, on the device.
        One kernel pass (phx_hill_jacobian, include/phoenix_hip.h): a forward-mode interpretation of the compiled programs,
        with fAct continued by 0 to TF <= 0 as `rhs` continues it."""
        if reduce not in JACOBIAN_MODES:
            raise ValueError('reduce must be None, "mean" or "mean_abs", got %r' % (reduce,))
        if not isinstance(x, torch.Tensor):
            raise TypeError("x must be a tensor on the GPU, got %s" % type(x).__name__)
        engine._require_gpu(x, "x")
        N = self.N
        if not ((x.dim() == 2 and x.shape[1] == N) or (x.dim() == 3 and x.shape[1:] == (1, N))) or x.shape[0] < 1:
            raise ValueError("x must be [B, %d] or [B, 1, %d], got %s" % (N, N, tuple(x.shape)))
        if self.device.type != "cuda" or x.device != self.code.device:
            raise ValueError("x is on %s, the system on %s" % (x.device, self.device))
        eptr, ereg, regulator, target = self._pattern_on_device()
        B, E, mode = x.shape[0], ereg.shape[0], JACOBIAN_MODES[reduce]
        value = torch.empty((B, E) if mode == 0 else (E,), dtype=torch.float32, device=x.device)
        if E == 0:                                       # input genes only: nothing to launch
            return HillJacobian(regulator, target, value)
        x2 = x.detach().reshape(B, N).contiguous()
        lib = _lib.load()
        nbytes = lib.phx_hill_jacobian_workspace_bytes(B, N, E, mode)
        ws = engine._stream_buffer(OP_HILL_JACOBIAN, nbytes, x.device, slack=256) if nbytes else None
        engine._check_call(lib.phx_hill_jacobian(*self._args(), engine._p(eptr), engine._p(ereg), engine._p(x2), B, N, E, mode,
                                                 engine._p(value), engine._p(ws), nbytes, engine._stream_ptr()))
        return HillJacobian(regulator, target, value)

    # ---- the attractors
    def block_structure(self):
        """The schedule of the steady-state solve, on the host from `jacobian_pattern()` with self-edges ignored:
        HillBlocks(order int32 [N], comp_ptr int32 [C + 1], level_ptr int32 [L + 1], largest).  The strongly connected
        components of the regulatory graph (an iterative Tarjan) are levelled at 1 + the highest level of a component that
        regulates them (0 without one; "input gene" rows are one-gene components at level 0); order lists the genes by
        component (ascending within one), the components by level (by their smallest gene within one);
        order[comp_ptr[c]:comp_ptr[c + 1]] is component c, components level_ptr[l]:level_ptr[l + 1] are level l; largest is
        the size of the largest component.  Every regulator of a gene lies in its own component or at a lower level, so
        apart from its diagonal the Jacobian is block lower triangular in `order`.  One schedule per system: a held or
        frozen gene only removes edges."""
        if self._blocks is None:
            pat, N = self.jacobian_pattern(), self.N
            regs = [[r for r in pat.regulator[pat.ptr[j]:pat.ptr[j + 1]].tolist() if r != j] for j in range(N)]
            # Tarjan on the graph target -> regulator: a component is finished after every component that regulates it
            index, low, comp = [-1] * N, [0] * N, [-1] * N
            on_stack, stack, comps, count = [False] * N, [], [], 0
            for root in range(N):
                if index[root] >= 0:
                    continue
                index[root] = low[root] = count
                count += 1
                stack.append(root)
                on_stack[root] = True
                work = [(root, 0)]
                while work:
                    v, i = work.pop()
                    if i < len(regs[v]):
                        work.append((v, i + 1))
                        w = regs[v][i]
                        if index[w] < 0:
                            index[w] = low[w] = count
                            count += 1
                            stack.append(w)
                            on_stack[w] = True
                            work.append((w, 0))
                        elif on_stack[w]:
                            low[v] = min(low[v], index[w])
                        continue
                    if low[v] == index[v]:
                        members = []
                        while True:
                            w = stack.pop()
                            on_stack[w] = False
                            comp[w] = len(comps)
                            members.append(w)
                            if w == v:
                                break
                        comps.append(sorted(members))
                    if work:
                        low[work[-1][0]] = min(low[work[-1][0]], low[v])
            level = []
            for c, members in enumerate(comps):        # in this order the regulators of a component come before it
                level.append(1 + max((level[comp[r]] for g in members for r in regs[g] if comp[r] != c), default=-1))
            by_level = sorted(range(len(comps)), key=lambda c: (level[c], comps[c][0]))
            order = np.asarray([g for c in by_level for g in comps[c]], np.int32)
            comp_ptr = np.zeros(len(comps) + 1, np.int32)
            np.cumsum([len(comps[c]) for c in by_level], out=comp_ptr[1:])
            n_level = max(level) + 1 if level else 0
            level_ptr = np.searchsorted(np.asarray([level[c] for c in by_level]), np.arange(n_level + 1)).astype(np.int32)
            self._blocks = HillBlocks(order, comp_ptr, level_ptr, max((len(m) for m in comps), default=0))
        return self._blocks

    def _blocks_on_device(self):
        """(order, comp_ptr, level_ptr) int32 of `block_structure()` on the system's device"""
        if self._blocks_dev is None:
            blk = self.block_structure()
            self._blocks_dev = tuple(torch.from_numpy(a).to(self.code.device) for a in blk[:3])
        return self._blocks_dev

    def _blocks_fit(self):
        """does phx_hill_steady take this system: no component above PHX_HILL_SCC_MAX, vectors within its LDS budget"""
        blk = self.block_structure()
        E = len(self.jacobian_pattern().regulator)
        return 1 <= blk.largest <= SCC_MAX and _lib.load().phx_hill_steady_lds_bytes(self.N, E, blk.largest) > 0

    def reached(self, gene):
        """bool [N] on the host: the genes whose rate depends on `gene` directly or through others (a graph search on
        `jacobian_pattern()` without its diagonal); `gene` itself only where a cycle leads back to it"""
        if self._targets_of is None:
            pat = self.jacobian_pattern()
            self._targets_of = [[] for _ in range(self.N)]
            for r, t in zip(pat.regulator.tolist(), pat.target.tolist()):
                if r != t:
                    self._targets_of[r].append(t)
        seen, todo = np.zeros(self.N, bool), [int(gene)]
        while todo:
            for t in self._targets_of[todo.pop()]:
                if not seen[t]:
                    seen[t] = True
                    todo.append(t)
        return seen

    def _steady_blocks(self, x, free, tol, max_iter, tau0):
        """phx_hill_steady on checked arguments: x [R, N] float32 contiguous, free [R, N] bool, both on the device"""
        R, N, dev = x.shape[0], self.N, x.device
        eptr, ereg = self._pattern_on_device()[:2]
        order, comp_ptr, level_ptr = self._blocks_on_device()
        moving = free.to(torch.uint8).contiguous()
        y = torch.empty_like(x)
        rho, tau = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
        its, status = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2))
        p = engine._p
        engine._check_call(_lib.load().phx_hill_steady(
            *self._args(), p(eptr), p(ereg), ereg.shape[0], p(order), p(comp_ptr), comp_ptr.shape[0] - 1, p(level_ptr),
            level_ptr.shape[0] - 1, self.block_structure().largest, p(x), p(moving), R, N, float(tol), int(max_iter), float(tau0),
            p(y), p(rho), p(its), p(status), p(tau), engine._stream_ptr()))
        return y, rho, its, status, tau

    def _steady_dense(self, x, free, tol, max_iter, tau0):
        """the same iteration from `rhs`, `jacobian` and a dense float64 solve of the N x N systems of all rows at once;
        control per row on the device as in `steady._iterate`, nothing is read back"""
        from . import steady
        B, N, dev = x.shape[0], self.N, x.device
        regulator, target = self._pattern_on_device()[2:]
        zero = x.new_zeros(())

        def rates(y):
            return torch.where(free, self.rhs(y), zero)

        f = rates(x)
        rho = f.abs().amax(dim=1)                                  # (amax hands a NaN on)
        tau = torch.full((B,), float(tau0), dtype=torch.float32, device=dev)
        status = torch.where(rho <= tol, steady.CONVERGED, steady.MAX_ITER).to(torch.int32)
        its = torch.zeros(B, dtype=torch.int32, device=dev)
        diag = torch.arange(N, device=dev)
        for _ in range(int(max_iter)):
            active = status == steady.MAX_ITER
            A = torch.zeros((B, N, N), dtype=torch.float64, device=dev)
            A[:, target, regulator] = -self.jacobian(x).value.double()
            A = A * free.unsqueeze(2)                              # a gene that does not move: the row of delta = 0
            A[:, diag, diag] += torch.where(free, (1 / tau).unsqueeze(1), x.new_ones(())).double()
            d, info = torch.linalg.solve_ex(A, f.double().unsqueeze(2))
            d = d.squeeze(2).float()
            bad = active & ((info != 0) | ~torch.isfinite(d).all(dim=1))
            xc = torch.where(free & (active & ~bad).unsqueeze(1), x + d, x)
            fc = rates(xc)
            rhoc = fc.abs().amax(dim=1)
            ok = active & ~bad & torch.isfinite(rhoc) & (rhoc <= 2 * rho)
            rejected = active & ~bad & ~ok
            tau = torch.where(ok, tau * torch.clamp(rho / rhoc, 2.0, 10.0), torch.where(rejected, tau / 4, tau))
            x = torch.where(ok.unsqueeze(1), xc, x)
            f = torch.where(ok.unsqueeze(1), fc, f)
            rho = torch.where(ok, rhoc, rho)
            its = its + active.to(torch.int32)
            status = torch.where(bad, steady.SINGULAR, torch.where(ok & (rhoc <= tol), steady.CONVERGED, status)).to(torch.int32)
        return x.clone() if int(max_iter) == 0 else x, rho, its, status, tau

    def _steady_control(self, name, tol, max_iter, tau0, method):
        """the checks of the control arguments, on the host -> the route, "blocks" or "dense" """
        from . import steady
        steady._check_control(name, tol, max_iter, tau0)
        if method not in (None, "blocks", "dense"):
            raise ValueError('%s: method must be None, "blocks" or "dense", got %r' % (name, method))
        if method == "dense":
            return method
        fits = self._blocks_fit()
        if method == "blocks" and not fits:
            raise ValueError("%s: method=\"blocks\" takes components of up to %d genes and a system whose vectors fit its "
                             "LDS; this one's largest component has %d of %d genes: use method=\"dense\""
                             % (name, SCC_MAX, self.block_structure().largest, self.N))
        return "blocks" if fits else "dense"

    def _steady_run(self, x, free, tol, max_iter, tau0, route, rows_per_call=None):
        from . import steady
        if len(self.jacobian_pattern().regulator) == 0:            # input genes only: nothing moves, nothing to launch
            B, dev = x.shape[0], x.device
            return steady.SteadyStates(x.clone(), torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                                       torch.zeros(B, dtype=torch.int32, device=dev),
                                       torch.full((B,), float(tau0), device=dev), None)
        if route == "blocks":
            step, run = steady.MAX_ROWS if rows_per_call is None else rows_per_call, self._steady_blocks
        else:
            step, run = max(1, min(steady.MAX_ROWS, steady.SOLVE_BYTES // (24 * self.N * self.N))), self._steady_dense
            step = step if rows_per_call is None else min(step, rows_per_call)
        parts = [run(x[r0:r0 + step], free[r0:r0 + step], float(tol), max_iter, tau0) for r0 in range(0, x.shape[0], step)]
        return steady.SteadyStates(*((torch.cat(c) for c in zip(*parts)) if len(parts) > 1 else parts[0]), None)

    def _moving(self, name, sets, frozen, B, device):
        """bool [B, N] on the device: gene n moves in row b -- it has a program, is not in the row's held set, not frozen"""
        free = np.repeat(~self.is_input[None, :], B, axis=0)
        for b, s in enumerate(sets):
            free[b, list(s)] = False
        if frozen is not None:
            free &= ~np.broadcast_to(frozen, free.shape)
        return torch.from_numpy(free).to(device)

    def _frozen(self, name, frozen, B):
        if frozen is None:
            return None
        fz = frozen.detach().cpu().numpy() if isinstance(frozen, torch.Tensor) else np.asarray(frozen)
        if fz.dtype != np.bool_ or fz.shape not in ((self.N,), (B, self.N)):
            raise ValueError("%s: frozen must be bool [%d] or [%d, %d], got %s %s" % (name, self.N, B, self.N, fz.dtype, fz.shape))
        return fz

    def steady_states(self, x0, clamp=None, frozen=None, tol=1e-5, max_iter=50, tau0=1.0, method=None):
        """The attractors of the system itself: the steady states the rows of x0 ([B, N] or [B, 1, N] float32 on the device)
        relax to -- the truth `steady.steady_states` of a model trained on this system's data is scored against.  A gene
        moves in row b if it has a rate expression, is not in row b's held set (`clamp`: per row up to four genes held at
        their x0 values, in the forms the model's function takes, -1 / () for none) and is not `frozen` (bool [B, N] or [N]);
        every other gene keeps its x0 bits.  The iteration and its control are those of the model's function, to the letter
        (rho = max |rate| over the moving genes; done at rho <= tol; a step of (I / tau - J) delta = f is accepted iff the new
        rho' is finite and <= 2 rho, then tau <- tau min(10, max(2, rho / rho')), else tau <- tau / 4; tau0 = inf: Newton).
        method="blocks": phx_hill_steady, one launch, a workgroup per row; a step is a forward substitution over the
        strongly connected components of the network (`block_structure()`), which must have at most 64 genes each; a row's
        bits depend on nothing but that row.  method="dense": the same iteration from `rhs`, `jacobian` and
        torch.linalg.solve_ex on [B, N, N] float64, rows in blocks within `steady.SOLVE_BYTES`; its bits may depend on the
        batch.  None: "blocks" where the system fits, else "dense".
        Returns `steady.SteadyStates(y, residual, iterations, status, tau, reduced=None)` of device tensors; status 0
        converged, 1 max_iter reached, 2 a zero or non-finite pivot or divisor.  Argument errors are raised on the host
        before any device call."""
        from . import steady
        name = "steady_states"
        route = self._steady_control(name, tol, max_iter, tau0, method)
        x2 = steady._rows(name, x0, self.N)
        B = x2.shape[0]
        sets = steady._held_sets(name, clamp, B, self.N)
        frozen = self._frozen(name, frozen, B)
        x2 = self._knockout_x0(name, x2)
        with torch.no_grad():
            return self._steady_run(x2, self._moving(name, sets, frozen, B, x2.device), tol, max_iter, tau0, route)

    def knockout_steady_states(self, x0, genes, value=0.0, rows_per_call=4096, **steady_kw):
        """Where does the SYSTEM settle when gene g is held at `value`: `steady.knockout_steady_states` on the simulator, the
        truth of that screen.  The unperturbed states of x0 are solved once; knockout k restarts from them with column
        genes[k] set to value[k] (a scalar or one level per gene) and held, and only the genes that genes[k] reaches
        (`reached`) move: a gene it does not reach cannot change and keeps the baseline's bits, so shift and magnitude are
        exactly 0 there.  The K B rows are solved in blocks of `rows_per_call`; steady_kw: tol, max_iter, tau0, method.
        Returns `steady.KnockoutSteadyStates(genes, base, knockouts, shift [K, N], magnitude [K, N])` as the model's."""
        from . import steady
        name, N = "knockout_steady_states", self.N
        if set(steady_kw) - {"tol", "max_iter", "tau0", "method"}:
            raise TypeError("%s: unexpected arguments %s" % (name, sorted(set(steady_kw) - {"tol", "max_iter", "tau0", "method"})))
        genes = engine.int_list(name, genes)
        engine.check_genes(name, genes, N)
        if not genes:
            raise ValueError("%s: no gene to hold" % name)
        values = engine.gene_values(name, value, len(genes))
        for v in values:
            if not np.isfinite(np.float32(v)):
                raise ValueError("%s: level %r is not a finite float32" % (name, v))
        if isinstance(rows_per_call, bool) or not hasattr(rows_per_call, "__index__") or int(rows_per_call) < 1:
            raise ValueError("%s: rows_per_call must be a positive integer" % name)
        kw = dict(dict(tol=1e-5, max_iter=50, tau0=1.0, method=None), **steady_kw)
        route = self._steady_control(name, kw["tol"], kw["max_iter"], kw["tau0"], kw["method"])
        x2 = self._knockout_x0(name, steady._rows(name, x0, N))
        B, K, dev = x2.shape[0], len(genes), x2.device
        with torch.no_grad():
            base = self._steady_run(x2, self._moving(name, [()] * B, None, B, dev), kw["tol"], kw["max_iter"], kw["tau0"], route)
            start = base.y.unsqueeze(0).repeat(K, 1, 1)
            free = np.zeros((K, N), bool)
            for k, (gene, v) in enumerate(zip(genes, values)):
                start[k, :, gene] = v
                free[k] = self.reached(gene) & ~self.is_input
                free[k, gene] = False
            free = torch.from_numpy(free).to(dev).unsqueeze(1).expand(K, B, N).reshape(K * B, N)
            ko = self._steady_run(start.reshape(K * B, N), free, kw["tol"], kw["max_iter"], kw["tau0"], route,
                                  min(int(rows_per_call), steady.MAX_ROWS))
            d = ko.y.reshape(K, B, N) - base.y.unsqueeze(0)
            shift, magnitude = d.mean(dim=1), d.abs().mean(dim=1)
        return steady.KnockoutSteadyStates(genes, base, ko, shift, magnitude)

    def sample_initial(self, numsamples, output_gene_var=1.0, rng=None, input_models=None, cor_strength=5.0,
                       input_gene_var=1.0, prop_bimodal=0.0):
        """Initial states of `simDataset` (SimulationGRN_core_init_var.R:165-213).  Regulated genes: Beta(2/var, 2/var)
        shifted by the gene's own U(-.25, .25), clipped to [0, 1] (R:206-213).  Input genes ("input gene" rows of the
        expression file, rate 0): drawn from their input models with rank-correlated unimodal inputs (R:177-184,
        `generate_input_data`); `input_models=None` creates the models first (`create_input_models`, R:32-34)."""
        rng = np.random.default_rng() if rng is None else rng
        a = 2.0 / output_gene_var
        x = rng.beta(a, a, size=(numsamples, self.N)) + rng.uniform(-0.25, 0.25, size=(1, self.N))
        x = np.clip(x, 0.0, 1.0)
        if self.is_input.any():
            in_names = [n for n, f in zip(self.names, self.is_input) if f]
            if input_models is None:
                input_models = create_input_models(in_names, prop_bimodal, rng)
            xin, self.last_input_classes = generate_input_data({n: input_models[n] for n in in_names}, numsamples,
                                                                cor_strength, input_gene_var, rng)
            x[:, self.is_input] = xin
        return x.astype(np.float32)


def jacobian_reference(system, x, dtype=np.float64, pattern=None):
    """`HillSystem.jacobian(x)` in numpy on the host, for a system on any device (device="cpu" included): [B, E] in `dtype`,
    entry (b, e) = d rate_target[e] / d x_regulator[e] at x[b] ([B, N] or [B, 1, N]) over `system.jacobian_pattern()` -- or
    over another `pattern` (a HillPattern; an entry whose regulator the target's program never pushes is +0).  The same
    forward-mode interpretation of the compiled programs as the kernel's, rule by rule (include/phoenix_hip.h), a target's
    regulators side by side.  dtype=np.float32 rounds states and constants first and runs every operation in float32, as
    `interpret_programs` of the oracle does for the rates: the rounding error a correct fp32 interpreter may show."""
    x = np.asarray(x, dtype)
    N = system.N
    if not ((x.ndim == 2 and x.shape[1] == N) or (x.ndim == 3 and x.shape[1:] == (1, N))) or x.shape[0] < 1:
        raise ValueError("x must be [B, %d] or [B, 1, %d], got %s" % (N, N, x.shape))
    x = x.reshape(x.shape[0], N)
    pat = system.jacobian_pattern() if pattern is None else pattern
    consts = np.asarray(system.consts_host, dtype)
    code, B = system.code_host.tolist(), x.shape[0]
    out = np.zeros((B, len(pat.regulator)), dtype)
    for j in range(N):
        e0, e1 = int(pat.ptr[j]), int(pat.ptr[j + 1])
        n = int(system.len_host[j])
        if e0 == e1 or n == 0:
            continue
        regs = np.asarray(pat.regulator[e0:e1])
        pushed = np.zeros(e1 - e0, bool)
        zero = np.zeros((B, e1 - e0), dtype)
        val, der = [], []                                  # [B] and [B, k]: one derivative column per regulator
        for op, arg in code[system.off_host[j]: system.off_host[j] + n]:
            if op == 0:
                val.append(np.full(B, consts[arg]))
                der.append(zero)
            elif op == 1:
                val.append(x[:, arg])
                der.append(np.broadcast_to((regs == arg).astype(dtype), zero.shape))
                pushed |= regs == arg
            elif op == 6:
                val[-1], der[-1] = -val[-1], -der[-1]
            elif op == 7:
                b, k, nn = consts[arg: arg + 3]
                tf, on = val[-1], val[-1] > 0
                tfp = np.where(on, np.abs(tf), dtype(1))
                tn = np.where(on, tfp ** nn, dtype(0))
                den = k + tn
                val[-1] = b * tn / den
                slope = np.where(on, b * k * nn * tfp ** (nn - dtype(1)) / (den * den), dtype(0))
                der[-1] = np.where(on[:, None], slope[:, None] * der[-1], dtype(0))
            else:
                r, rd = val.pop(), der.pop()
                l, ld = val[-1], der[-1]
                if op == 2:
                    val[-1], der[-1] = l + r, ld + rd
                elif op == 3:
                    val[-1], der[-1] = l - r, ld - rd
                elif op == 4:
                    val[-1], der[-1] = l * r, ld * r[:, None] + l[:, None] * rd
                else:
                    q = l / r
                    val[-1], der[-1] = q, (ld - q[:, None] * rd) / r[:, None]
        out[:, e0:e1] = np.where(pushed[None, :], der[0], dtype(0))
    return out


def _program_shapes(system):
    """the programs of a system grouped by their opcode sequence: [(ops tuple, genes int64 [G], args int64 [len, G])];
    genes of one shape are interpreted side by side"""
    shapes = getattr(system, "_shapes", None)
    if shapes is None:
        by_ops = {}
        for g in range(system.N):
            o, n = int(system.off_host[g]), int(system.len_host[g])
            if n:
                by_ops.setdefault(tuple(system.code_host[o:o + n, 0].tolist()), []).append(g)
        shapes = system._shapes = [
            (ops, np.asarray(gs, np.int64),
             np.stack([system.code_host[system.off_host[g]: system.off_host[g] + len(ops), 1] for g in gs], 1).astype(np.int64))
            for ops, gs in by_ops.items()]
    return shapes


def rates_reference(system, x, dtype=np.float64):
    """`HillSystem.rhs(x)` in numpy on the host, for a system on any device (device="cpu" included): the rates at the states
    x [..., N] in `dtype`, "input gene" rows 0.  The value half of `jacobian_reference`'s interpreter -- the compiled programs
    operation by operation, fAct continued by 0 at TF <= 0 -- with the genes whose programs have the same opcode sequence
    evaluated side by side (the same elementwise arithmetic as gene by gene).  dtype=np.float32 rounds states and constants
    first and runs every operation in float32."""
    x = np.asarray(x, dtype)
    if x.ndim < 1 or x.shape[-1] != system.N:
        raise ValueError("x must be [..., %d], got %s" % (system.N, x.shape))
    rows = x.reshape(-1, system.N)
    consts = np.asarray(system.consts_host, dtype)
    out = np.zeros_like(rows)
    for ops, genes, args in _program_shapes(system):
        st = []
        for i, op in enumerate(ops):
            a = args[i]
            if op == 0:
                st.append(np.broadcast_to(consts[a], (rows.shape[0], len(genes))))
            elif op == 1:
                st.append(rows[:, a])
            elif op == 6:
                st[-1] = -st[-1]
            elif op == 7:
                b, k, nn = consts[a], consts[a + 1], consts[a + 2]
                tf, on = st[-1], st[-1] > 0
                tn = np.where(on, np.where(on, np.abs(tf), dtype(1)) ** nn, dtype(0))
                st[-1] = b * tn / (k + tn)
            else:
                r = st.pop()
                l = st[-1]
                st[-1] = l + r if op == 2 else l - r if op == 3 else l * r if op == 4 else l / r
        out[:, genes] = st[0]
    return out.reshape(x.shape)


def knockouts_reference(system, x0, times, genes, values, dt_max, dtype=np.float64):
    """`HillSystem.knockouts` in numpy on the host, for a system on any device: [T, K, B, N] in `dtype`.  A restatement of
    the kernel's integrator on `rates_reference` -- classical RK4 in the kernel's order of operations, nsub = max(1,
    ceil(|span| / dt_max)) equal sub-steps of h = dtype(span / nsub) per interval -- with the clamp: call k starts with
    column genes[k] at values[k], and the rate of that column is replaced by 0 in every stage (genes[k] == -1: none).
    x0 [B, N] or [B, 1, N]; genes / values: K ints in -1 .. N - 1 and K levels -- or, as in `HillSystem.knockouts`, sets of
    up to 4 genes with a level, or a sequence of levels, per call: every column of a set starts at its level and has rate 0."""
    N = system.N
    x0 = np.asarray(x0, dtype)
    if not ((x0.ndim == 2 and x0.shape[1] == N) or (x0.ndim == 3 and x0.shape[1:] == (1, N))) or x0.shape[0] < 1:
        raise ValueError("x0 must be [B, %d] or [B, 1, %d], got %s" % (N, N, x0.shape))
    if _names_sets(genes):
        sets, levels = _knockout_set_args("knockouts_reference", N, genes, values)
    else:
        genes, values = _knockout_args("knockouts_reference", N, genes, values if np.isscalar(values) else list(values), lowest=-1)
        sets, levels = [(g,) if g >= 0 else () for g in genes], [(v,) for v in values]
    t64, dt_max = _knockout_times("knockouts_reference", times, dt_max)
    K, B = len(sets), x0.shape[0]
    y = np.repeat(x0.reshape(1, B, N), K, axis=0)
    held = [(k, g) for k in range(K) for g in sets[k]]
    for k in range(K):
        for g, v in zip(sets[k], levels[k]):
            y[k, :, g] = dtype(v)

    def f(x):
        r = rates_reference(system, x, dtype)
        for k, g in held:
            r[k, :, g] = 0
        return r

    out = [y.copy()]
    half, one, two, six = dtype(0.5), dtype(1), dtype(2), dtype(6)
    for i in range(len(t64) - 1):
        span = t64[i + 1] - t64[i]
        nsub = max(1, int(np.ceil(abs(span) / dt_max)))
        h = dtype(span / nsub)
        for _ in range(nsub):
            k1 = f(y)
            acc = one * k1
            k2 = f(y + (half * h) * k1)
            acc = acc + two * k2
            k3 = f(y + (half * h) * k2)
            acc = acc + two * k3
            k4 = f(y + h * k3)
            acc = acc + one * k4
            y = y + (h / six) * acc
        out.append(y.copy())
    return np.stack(out)


def _lu_solve(A, b):
    """A x = b in float64 by LU with partial pivoting as phx_hill_steady does it (the first largest |a| of a column, a NaN
    wins; elimination by rows, back substitution by columns) -> (x, bad): bad for a pivot that is 0 or not finite"""
    A, b = np.array(A, np.float64), np.array(b, np.float64)
    n = len(b)
    with np.errstate(all="ignore"):
        for k in range(n):
            col = A[k:, k]
            key = np.where(np.isnan(col), np.inf, np.abs(col))
            p = k + int(np.argmax(key))
            if not key[p - k] > 0 or np.isinf(key[p - k]):
                return np.zeros(n), True
            if p != k:
                A[[k, p]] = A[[p, k]]
                b[[k, p]] = b[[p, k]]
            fac = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] -= fac[:, None] * A[k, k + 1:][None, :]
            b[k + 1:] -= fac * b[k]
        for k in range(n - 1, -1, -1):
            b[k] = b[k] / A[k, k]
            b[:k] -= A[:k, k] * b[k]
    return b, False


def block_substitution(system, J, f, sigma, moving=None, dtype=np.float64):
    """(sigma I - J) delta = f of ONE state by the forward substitution of phx_hill_steady over `system.block_structure()`,
    in numpy: J [E] on `system.jacobian_pattern()`, f [N]; a one-gene component is delta_j = (f_j + sum_{k != j} J_jk
    delta_k) / (sigma - J_jj) in `dtype`, the row's entries ascending; a larger one assembles its block in float64 and solves
    it by LU with partial pivoting (`_lu_solve`).  A gene with moving[n] false has delta 0 whatever J and f say.
    Returns (delta [N] in `dtype`, bad): bad for a pivot or a divisor that is 0 or not finite."""
    dt = np.dtype(dtype).type
    blk, pat, N = system.block_structure(), system.jacobian_pattern(), system.N
    moving = np.ones(N, bool) if moving is None else np.asarray(moving, bool)
    J, f, sigma = np.asarray(J, dt), np.asarray(f, dt), dt(sigma)
    order, ptr, reg = blk.order.tolist(), pat.ptr.tolist(), pat.regulator.tolist()
    pos = np.empty(N, np.int64)
    pos[blk.order] = np.arange(N)
    d, bad = np.zeros(N, dt), False
    with np.errstate(all="ignore"):
        for c in range(len(blk.comp_ptr) - 1):              # by level: every regulator outside the component is done
            o, n = int(blk.comp_ptr[c]), int(blk.comp_ptr[c + 1] - blk.comp_ptr[c])
            if n == 1:
                g = order[o]
                if not moving[g]:
                    continue
                acc, jd = f[g], dt(0)
                for e in range(ptr[g], ptr[g + 1]):
                    if reg[e] == g:
                        jd = J[e]
                    else:
                        acc = acc + J[e] * d[reg[e]]
                div = sigma - jd
                bad = bad or not abs(div) > 0 or bool(np.isinf(div))
                d[g] = acc / div
                continue
            A, b = np.zeros((n, n)), np.zeros(n)
            for i, g in enumerate(order[o:o + n]):
                if not moving[g]:
                    A[i, i] = 1.0
                    continue
                A[i, i] = float(sigma)
                acc = float(f[g])
                for e in range(ptr[g], ptr[g + 1]):
                    rk = int(pos[reg[e]]) - o
                    if 0 <= rk < n:
                        A[i, rk] -= float(J[e])
                    else:
                        acc += float(J[e]) * float(d[reg[e]])
                b[i] = acc
            x, singular = _lu_solve(A, b)
            bad = bad or singular
            d[order[o:o + n]] = x.astype(dt)
    return d, bad


def steady_states_reference(system, x0, clamp=None, frozen=None, tol=1e-5, max_iter=50, tau0=1.0, dtype=np.float64,
                            solve="dense"):
    """`HillSystem.steady_states` in numpy on the host, for a system on any device: the same iteration and control on
    `rates_reference` / `jacobian_reference` in `dtype`.  solve="blocks" restates the kernel's level-by-level substitution
    (`block_substitution`); solve="dense" solves the N x N system (rows of genes that do not move replaced by delta = 0) with
    np.linalg.solve in float64.  x0 [B, N] or [B, 1, N]; clamp, frozen as there.  Returns `steady.SteadyStates` of numpy
    arrays, reduced None."""
    from . import steady
    name = "steady_states_reference"
    steady._check_control(name, tol, max_iter, tau0)
    if solve not in ("dense", "blocks"):
        raise ValueError('%s: solve must be "dense" or "blocks", got %r' % (name, solve))
    dt = np.dtype(dtype).type
    N = system.N
    x = np.array(x0, dtype=dt)
    if not ((x.ndim == 2 and x.shape[1] == N) or (x.ndim == 3 and x.shape[1:] == (1, N))) or x.shape[0] < 1:
        raise ValueError("%s: x0 must be [B, %d] or [B, 1, %d], got %s" % (name, N, N, x.shape))
    x = x.reshape(x.shape[0], N)
    B = x.shape[0]
    free = system._moving(name, steady._held_sets(name, clamp, B, N), system._frozen(name, frozen, B), B, "cpu").numpy()
    pat = system.jacobian_pattern()
    row_moves = free[:, pat.target]                           # [B, E]: the entry's target moves

    def state(y):
        with np.errstate(all="ignore"):
            f = np.where(free, rates_reference(system, y, dt), dt(0))
            return f, np.abs(f).max(axis=1)

    f, rho = state(x)
    tau = np.full(B, tau0, dt)
    status = np.where(rho <= tol, steady.CONVERGED, steady.MAX_ITER).astype(np.int32)
    its = np.zeros(B, np.int32)
    for _ in range(int(max_iter)):
        active = status == steady.MAX_ITER
        if not active.any():
            break
        xc, bad = x.copy(), np.zeros(B, bool)
        with np.errstate(all="ignore"):
            J = np.where(row_moves, jacobian_reference(system, x, dt), dt(0))
            sigma = (1 / tau).astype(dt)
            for b in np.nonzero(active)[0]:
                if solve == "blocks":
                    d, bad[b] = block_substitution(system, J[b], f[b], sigma[b], free[b], dt)
                else:
                    A = np.zeros((N, N))
                    A[pat.target, pat.regulator] = -J[b].astype(np.float64)
                    A[np.arange(N), np.arange(N)] += np.where(free[b], float(sigma[b]), 1.0)
                    try:
                        if not np.all(np.isfinite(A)):
                            raise np.linalg.LinAlgError
                        d = np.linalg.solve(A, f[b].astype(np.float64)).astype(dt)
                        if not np.all(np.isfinite(d)):
                            raise np.linalg.LinAlgError
                    except np.linalg.LinAlgError:
                        bad[b] = True
                if not bad[b]:
                    xc[b] = np.where(free[b], x[b] + d, x[b])
            fc, rhoc = state(xc)
            ok = active & ~bad & np.isfinite(rhoc) & (rhoc <= 2 * rho)
            rejected = active & ~bad & ~ok
            grow = np.clip(rho / np.where(rhoc > 0, rhoc, dt(1e-300) if dt is np.float64 else dt(1e-45)), 2, 10).astype(dt)
            tau = np.where(ok, tau * grow, np.where(rejected, tau / 4, tau)).astype(dt)
        x[ok], f[ok], rho[ok] = xc[ok], fc[ok], rhoc[ok]
        its += active
        status = np.where(bad, steady.SINGULAR, np.where(ok & (rhoc <= tol), steady.CONVERGED, status)).astype(np.int32)
    return steady.SteadyStates(x, rho, its, status, tau, None)


def generate_dataset(system, numsamples, time_stamps=(0.0, 2.0, 3.0, 7.0, 9.0), expnoise=0.0, dt_max=0.01, rng=None,
                     path=None, derivative=False, **initial_kw):
    """One in-silico data set like the reference's `example_creator...R` run: `numsamples` trajectories at
    `time_stamps` (example_creator_for_chalmers_codebase_0noise.R:134-139), optional Gaussian measurement noise
    (`addNormNoise`, SimulationGRN_core_init_var.R:1-3, 260-265); written with `writecsv` if `path` is given.
    `derivative=True` is the reference's `get_derivative_instead` branch (R:222-240): the table holds the rates at the
    solution's states instead of the states, and zeros in the input columns.  `initial_kw` goes to
    `HillSystem.sample_initial` (input models, `cor_strength`, `input_gene_var`, `output_gene_var`, `prop_bimodal`).
    Returns (data_np, t_np) in `readcsv`'s shapes."""
    from .data import writecsv
    rng = np.random.default_rng() if rng is None else rng
    x0 = torch.from_numpy(system.sample_initial(numsamples, rng=rng, **initial_kw)).to(system.device)
    sol = system.simulate(x0, time_stamps, dt_max)                          # [T, S, N]
    if derivative:
        sol = system.rhs(sol.reshape(-1, system.N)).reshape(sol.shape)      # rate 0 for input genes = the zero columns
    sol = sol.cpu().numpy()
    if expnoise > 0:
        sol = sol + rng.normal(0.0, expnoise, size=sol.shape).astype(np.float32)
    data_np = [sol[:, s].reshape(len(time_stamps), 1, system.N) for s in range(numsamples)]
    t_np = [np.asarray(time_stamps, np.float64) for _ in range(numsamples)]
    if path is not None:
        writecsv(path, system.N, numsamples, data_np, t_np)
    return data_np, t_np
