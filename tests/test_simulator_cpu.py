"""Row f4: compiler of the Hill-kinetics rate expressions (host logic) against golden G11 =
Python's own fp64 evaluation of the shipped 350-gene expression strings."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden



def _system(g, device, tmp_path=None):
    """HillSystem of the fixture's 350-gene network; through the CSV wire format when a directory is given."""
    from phoenix_amd.simulator import HillSystem
    names, eqns = [str(x) for x in g["names"]], [str(x) for x in g["eqns"]]
    if tmp_path is None:
        return HillSystem(names, eqns, device=device)
    import csv
    path = os.path.join(str(tmp_path), "ode_system.csv")
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, quoting=csv.QUOTE_ALL)
        w.writerow(["node", "eqn"])
        w.writerows(zip(names, eqns))
    return HillSystem.from_csv(path, device=device)


@pytest.mark.parametrize("fixture,N,n_input", [("g11_hill", 350, 74), ("g13_hill690", 690, None)])
def test_compiled_programs_match_the_expression_strings(tmp_path, fixture, N, n_input):
    """both shipped networks (ode_system_functions_350.csv / _690.csv): 74 "input gene" rows in the 350-gene one"""
    g = load_golden(fixture)
    sys_ = _system(g, "cpu", tmp_path)
    assert sys_.N == N
    if n_input is None:
        n_input = sum(1 for e in g["eqns"] if "input gene" in str(e))
        assert n_input > 0
    assert int(sys_.is_input.sum()) == n_input
    from oracle import hill_oracle
    got = hill_oracle.interpret_programs(sys_.code_host, sys_.consts_host, sys_.off_host, sys_.len_host, g["X"])
    assert np.max(np.abs(got - g["rates"])) < 1e-12
    assert np.all(got[:, sys_.is_input] == 0)


def test_oracle_fact_matches_the_r_definition():
    from oracle import hill_oracle
    from phoenix_amd.simulator import fact_constants
    # GraphGRN_core.R:431-436 at the default parameters and at one shipped edge
    for ec50, n, tf in ((0.5, 1.39, 0.3), (0.408142132172361, 1.79729779304471, 0.9)):
        b, k, _ = fact_constants(ec50, n)
        assert abs(hill_oracle.fAct(tf, ec50, n) - b * tf ** n / (k + tf ** n)) < 1e-15
    assert abs(hill_oracle.fAct(1.0, 0.5, 1.39) - 1.0) < 1e-12          # saturates at TF = 1


def test_unsupported_syntax_is_rejected():
    from phoenix_amd.simulator import HillSystem
    with pytest.raises(ValueError):
        HillSystem(["A", "B"], ["A ** 2", "input gene"], device="cpu")
    with pytest.raises(ValueError):
        HillSystem(["A", "B"], ["fAct(C, 0.5, 1.2) - A", "input gene"], device="cpu")


@pytest.mark.gpu
def test_hill_690_gene_network_on_device():
    """the second shipped expression file (690 nodes): phx_hill_rhs / phx_hill_simulate against golden G13"""
    g = load_golden("g13_hill690")
    dev = torch.device("cuda:0")
    sys_ = _system(g, dev)
    assert sys_.N == 690
    rates = sys_.rhs(torch.from_numpy(g["X"]).float().to(dev)).cpu().numpy()
    assert np.max(np.abs(rates - g["rates"])) < 5e-6
    traj = sys_.simulate(torch.from_numpy(g["x0"]).float().to(dev), g["times"]).cpu().numpy()
    assert traj.shape == g["traj"].shape
    assert np.max(np.abs(traj - g["traj"])) / np.max(np.abs(g["traj"])) < 1e-5
    assert np.array_equal(traj[-1][:, sys_.is_input], traj[0][:, sys_.is_input])


@pytest.mark.gpu
def test_hill_rhs_and_trajectories_on_device(tmp_path):
    """phx_hill_rhs / phx_hill_simulate (fp32, RK4 sub-steps of 0.01) against the fp64 oracle values."""
    from phoenix_amd.data import readcsv
    from phoenix_amd.simulator import generate_dataset
    g = load_golden("g11_hill")
    dev = torch.device("cuda:0")
    sys_ = _system(g, dev)
    rates = sys_.rhs(torch.from_numpy(g["X"]).float().to(dev)).cpu().numpy()
    assert np.max(np.abs(rates - g["rates"])) < 5e-6
    traj = sys_.simulate(torch.from_numpy(g["x0"]).float().to(dev), g["times"]).cpu().numpy()
    assert traj.shape == g["traj"].shape
    assert np.max(np.abs(traj - g["traj"])) / np.max(np.abs(g["traj"])) < 1e-5
    assert np.array_equal(traj[0], g["x0"].astype(np.float32))
    # input genes stay constant; a generated data set round-trips through the reference's CSV wire format
    assert np.array_equal(traj[-1][:, sys_.is_input], traj[0][:, sys_.is_input])
    path = str(tmp_path / "sim.csv")
    data_np, t_np = generate_dataset(sys_, 5, rng=np.random.default_rng(3), path=path)
    np.random.seed(0)
    back = readcsv(path, "cpu", 0.0, 1.0)
    assert back[4] == 350 and back[5] == 5
    assert np.allclose(back[0][2], data_np[2], rtol=0, atol=1e-6) and np.array_equal(back[2][0], t_np[0])
    assert all(np.all((d >= -1e-4) & (d <= 1.0 + 1e-4)) for d in data_np)   # Hill dynamics keep expression in [0, 1]
    # the reference's `get_derivative_instead` branch (SimulationGRN_core_init_var.R:222-240): rates at the solution's
    # states, zeros in the input columns; same draws => same underlying states
    ddata, _ = generate_dataset(sys_, 5, rng=np.random.default_rng(3), derivative=True)
    want = sys_.rhs(torch.from_numpy(np.stack(data_np)).to(dev).reshape(-1, 350)).cpu().numpy().reshape(5, -1, 1, 350)
    assert np.max(np.abs(np.stack(ddata) - want)) < 1e-6
    assert np.all(np.stack(ddata)[..., sys_.is_input] == 0)


# --------------------------------------------------------------------------- external inputs of a simulated data set
def test_input_models_follow_the_reference_recipe():
    """createInputModels (SimulationGRN_core_init_var.R:40-68): structure and ranges of the mixtures."""
    from phoenix_amd.simulator import create_input_models
    rng = np.random.default_rng(3)
    names = ["g%d" % i for i in range(400)]
    m = create_input_models(names, prop_bimodal=0.3, rng=rng)
    nb = 0
    for n in names:
        k = len(m[n]["prop"])
        assert k in (1, 2) and len(m[n]["mean"]) == k and len(m[n]["sd"]) == k
        assert abs(m[n]["prop"].sum() - 1.0) < 1e-12
        assert np.all(m[n]["mean"] > 0) and np.all(m[n]["mean"] < 1)
        assert np.all(m[n]["sd"] >= 0.01) and np.all(m[n]["sd"] <= np.maximum(np.minimum(m[n]["mean"], 1 - m[n]["mean"]) / 3, 0.01))
        if k == 2:
            nb += 1
            assert 0.2 <= m[n]["prop"][0] <= 0.8
    assert 0.2 < nb / len(names) < 0.4                       # sample(c(1,2), prob = c(1-p, p))
    low = np.mean([m[n]["mean"][0] for n in names if len(m[n]["prop"]) == 2])
    assert 0.05 < low < 0.14                                 # Beta(10, 100) has mean 1/11
    assert all(len(v["prop"]) == 1 for v in create_input_models(names, 0.0, rng).values())


def test_vine_correlation_matrices_are_correlation_matrices():
    """vineS (R:76-98): symmetric, unit diagonal, positive semi-definite; smaller beta = stronger correlations."""
    from phoenix_amd.simulator import vine_correlation
    rng = np.random.default_rng(0)
    strength = {}
    for beta in (0.5, 5.0, 50.0):
        vals = []
        for _ in range(5):
            S = vine_correlation(12, beta, rng)
            assert np.allclose(S, S.T) and np.allclose(np.diag(S), 1.0)
            assert np.linalg.eigvalsh(S).min() > -1e-10
            assert np.abs(S).max() <= 1.0 + 1e-12
            vals.append(np.abs(S[np.triu_indices(12, 1)]).mean())
        strength[beta] = np.mean(vals)
    assert strength[0.5] > strength[5.0] > strength[50.0]
    assert np.array_equal(vine_correlation(2, 5.0, rng), np.eye(2))


def test_generated_inputs_keep_their_marginals_and_gain_rank_correlation():
    """generateInputData (R:101-160): values in [0,1]; the correlation step only PERMUTES the draws of a unimodal input
    (rank matching), never touches a bimodal one, and produces the rank correlation of the vine matrix."""
    from phoenix_amd.simulator import create_input_models, generate_input_data
    names = ["in%d" % i for i in range(8)]
    models = create_input_models(names, prop_bimodal=0.4, rng=np.random.default_rng(5))
    X0, c0 = generate_input_data(models, 4000, cor_strength=0.0, rng=np.random.default_rng(11))
    X1, c1 = generate_input_data(models, 4000, cor_strength=0.7, rng=np.random.default_rng(11))
    assert X0.shape == X1.shape == (4000, 8)
    assert X0.min() >= 0 and X0.max() <= 1 and X1.min() >= 0 and X1.max() <= 1
    assert set(c0) == set(c1) == {n for n in names if len(models[n]["prop"]) == 2}
    for c, n in enumerate(names):
        if n in c1:
            assert np.array_equal(X0[:, c], X1[:, c])                        # bimodal: own draws (same generator state)
            assert np.array_equal(c0[n], c1[n]) and set(np.unique(c1[n])) <= {1, 2}
            lo = X1[c1[n] == 1, c].mean()
            assert abs(lo - models[n]["mean"][0]) < 0.05
        else:
            assert np.array_equal(np.sort(X0[:, c]), np.sort(X1[:, c]))      # unimodal: a permutation of the same draws
            assert abs(X1[:, c].mean() - models[n]["mean"][0]) < 0.05
    uni = [c for c, n in enumerate(names) if n not in c1]
    if len(uni) >= 2:
        def spearman(a, b):
            ra, rb = np.argsort(np.argsort(a)), np.argsort(np.argsort(b))
            return np.corrcoef(ra, rb)[0, 1]
        before = max(abs(spearman(X0[:, i], X0[:, j])) for i in uni for j in uni if i < j)
        after = max(abs(spearman(X1[:, i], X1[:, j])) for i in uni for j in uni if i < j)
        assert before < 0.08 < after


def test_initial_states_use_the_input_models_for_input_genes():
    from phoenix_amd.simulator import HillSystem
    names = ["A", "B", "C", "D"]
    exprs = ["input gene", "(0.5 * A) - (0.3 * B)", "input gene", "(0.2 * C) - (0.1 * D)"]
    sysm = HillSystem(names, exprs, device="cpu")
    x = sysm.sample_initial(500, rng=np.random.default_rng(1), prop_bimodal=0.0, cor_strength=0.0)
    assert x.shape == (500, 4) and x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1
    # input genes: one truncated normal each (tight), regulated genes: Beta(2,2) + shift (wide)
    assert x[:, 0].std() < 0.17 and x[:, 2].std() < 0.17 and x[:, 1].std() > 0.17 and x[:, 3].std() > 0.17


def _edges(tag):
    g = load_golden("g16_edges")
    cols = {k: g["e%s_%s" % (tag, k)] for k in ("from", "to", "weight", "activation", "EC50", "n")}
    return {(str(f), str(t)): {k: str(cols[k][i]) for k in cols}
            for i, (f, t) in enumerate(zip(cols["from"], cols["to"]))}


def test_equation_builder_reproduces_the_shipped_expressions_text_for_text():
    """Row f4, the equation-builder half (GraphGRN_core.R:163-190 NODE / NOT / AND / OR, :221-236 generateRateEqn_modified,
    :312-330 the activation term): `simulator.rate_expression(logic, edge table)` rebuilds EVERY non-input row of the shipped
    ode_system_functions_350.csv (golden G11) character for character from the shipped edge_properties_G350.csv (golden
    G16: weights, EC50 and Hill constants as R printed them), and an edge sits under a NOT exactly where its
    `activation` flag is FALSE.  The logic equations themselves are random draws of the reference's graph construction
    (genericLogicEqn, R:727-800) that are not shipped: they are recovered from the expression text."""
    from phoenix_amd import simulator as sim
    g = load_golden("g11_hill")
    edges = _edges("350")
    n, used = 0, set()
    for node, eqn in zip(g["names"], g["eqns"]):
        node, eqn = str(node), str(eqn)
        if eqn == "input gene":
            continue
        tree, spmax, spdeg, tau, leaves = sim.logic_of_expression(eqn, node)
        assert sim.rate_expression(node, tree, edges, spmax, spdeg, tau) == eqn, node
        for tf, w, ec50, hill, neg in leaves:
            e = edges[(tf, node)]
            used.add((tf, node))
            assert (e["weight"], e["EC50"], e["n"]) == (w, ec50, hill) and (e["activation"] == "FALSE") == neg, (tf, node)
        n += 1
    assert n == 276 and len(used) >= 547          # every rate expression; all but three of the 550 shipped edges occur


def test_equation_structure_of_the_690_gene_network_matches_its_edge_table():
    """The shipped edge_properties_G690.csv is NOT the table the shipped 690-gene expressions were printed from (every
    EC50 / n differs: another draw), so only the structure can be held there: every regulator in an expression is an edge
    of the table, negated exactly where `activation` is FALSE, and the builder reproduces each expression from its own
    constants."""
    from phoenix_amd import simulator as sim
    g = load_golden("g13_hill690")
    edges = _edges("690")
    n = 0
    for node, eqn in zip(g["names"], g["eqns"]):
        node, eqn = str(node), str(eqn)
        if eqn == "input gene":
            continue
        tree, spmax, spdeg, tau, leaves = sim.logic_of_expression(eqn, node)
        own = {(tf, node): {"from": tf, "weight": w, "EC50": ec50, "n": hill} for tf, w, ec50, hill, _ in leaves}
        assert sim.rate_expression(node, tree, own, spmax, spdeg, tau) == eqn, node
        for tf, _w, _e, _h, neg in leaves:
            assert (edges[(tf, node)]["activation"] == "FALSE") == neg, (tf, node)
        n += 1
    assert n == 593


# --------------------------------------------------------------------------- synthetic networks (shared with
# tests/test_simulator_gpu.py): any size, from the project's own equation builder, plus two hand-written genes for what
# the shipped text never has -- the deepest evaluation stack the device interpreter holds, and the unary operators
CHAIN = 24          # activations of the deep gene = MAX_STACK (HILL_STACK in csrc/phx_hill.inc)
_NETWORKS = {}


def and_chain(node, regulators, edges):
    """right-nested AND over the regulators: (a1 * (a2 * (... * aL)))"""
    tree = ("node", regulators[-1])
    for tf in reversed(regulators[:-1]):
        tree = ("and", ("node", tf), tree)
    return tree


def compiled_depth(names, expr):
    import ast
    from phoenix_amd.simulator import _Compiler
    c = _Compiler({n: i for i, n in enumerate(names)})
    c.visit(ast.parse(expr, mode="eval"))
    return c.max_depth, len(c.code)


def synthetic_network(N, seed=0):
    """Seeded N-gene network: about 20 % "input gene" rows; every other gene gets 1-4 random regulators joined by random
    and / or / not, written by `simulator.rate_expression`; edge weights U(0.5, 1), n U(1.39, 3), EC50 U(0.25, 0.5), so
    EC50^n < 0.45, K_n > 0 and K_n + TF^n cannot vanish.  The last two genes are hand-written: `DEEP`, a right-nested AND
    chain of CHAIN activations (weight 1) of the genes `info["chain_regs"]`, which needs an evaluation stack of exactly
    MAX_STACK, and `UNARY`, whose text has unary minus (of a constant and of a term), unary plus and a division by a
    constant.  Returns (names, expressions, info); cached, the lists are not to be modified."""
    if (N, seed) in _NETWORKS:
        return _NETWORKS[(N, seed)]
    from phoenix_amd import simulator as sim
    assert N >= 12
    rs = np.random.RandomState(500 + seed + N)
    names = ["G%d" % i for i in range(N - 2)] + ["DEEP", "UNARY"]
    is_input = rs.rand(N) < 0.2
    is_input[N - 2:] = False
    edges = {}

    def edge(tf, node, weight=None):
        w, n, ec50 = rs.uniform(0.5, 1.0), rs.uniform(1.39, 3.0), rs.uniform(0.25, 0.5)
        assert ec50 ** n < 0.45 and sim.fact_constants(ec50, n)[1] > 0            # K_n > 0
        edges[(tf, node)] = {"from": tf, "weight": weight or "%.9g" % w, "EC50": "%.9g" % ec50, "n": "%.9g" % n}

    def logic(regs):
        t = ("node", regs[0]) if rs.rand() < 0.7 else ("not", ("node", regs[0]))
        for tf in regs[1:]:
            u = ("node", tf) if rs.rand() < 0.7 else ("not", ("node", tf))
            t = ("and" if rs.rand() < 0.5 else "or", t, u) if rs.rand() < 0.5 else ("or" if rs.rand() < 0.5 else "and", u, t)
            if rs.rand() < 0.15:
                t = ("not", t)
        return t

    exprs = []
    for g in range(N - 2):
        if is_input[g]:
            exprs.append("input gene")
            continue
        regs = [names[i] for i in np.unique(rs.randint(0, N, rs.randint(1, 5)))]      # itself, DEEP and UNARY included
        for tf in regs:
            edge(tf, names[g])
        exprs.append(sim.rate_expression(names[g], logic(regs), edges))
    chain_regs = [names[i] for i in rs.choice(N - 2, CHAIN, replace=N - 2 < CHAIN)]   # a tiny network repeats some
    for tf in chain_regs:
        edge(tf, "DEEP", weight="1")
    exprs.append(sim.rate_expression("DEEP", and_chain("DEEP", chain_regs, edges), edges))
    a, b = names[int(rs.randint(0, N - 2))], names[int(rs.randint(0, N - 2))]
    exprs.append("(-(-0.9 * fAct(%s, 0.31, 2.2) + +%s) / 2.5 + 0.6 - UNARY) / 1.25" % (a, b))
    assert compiled_depth(names, exprs[N - 2]) == (sim.MAX_STACK, 127) and CHAIN == sim.MAX_STACK
    info = {"is_input": is_input, "chain_regs": np.array([names.index(t) for t in chain_regs]), "deep": N - 2,
            "unary": N - 1}
    from oracle import hill_oracle
    rates = hill_oracle.rhs(names, exprs, synthetic_states(N, 3, info, seed), fact=hill_oracle.fAct0)
    assert np.all(np.isfinite(rates)) and np.all(rates[:, is_input] == 0)
    assert 0.15 < is_input.mean() < 0.25 or N < 200
    _NETWORKS[(N, seed)] = (names, exprs, info)
    return names, exprs, info


def synthetic_states(N, B, info, seed=0):
    """fp32 states from U(-0.2, 1.2), so that TF <= 0 (fAct = 0 there) and TF > 1 both occur; the regulators of DEEP are
    drawn from U(0.8, 1.2) instead: with one factor of its 24-fold product at zero in six rows of seven, the deep gene
    would test nothing"""
    rs = np.random.RandomState(900 + seed + N + 13 * B)
    x = rs.uniform(-0.2, 1.2, (B, N))
    x[:, info["chain_regs"]] = rs.uniform(0.8, 1.2, (B, CHAIN))
    return x.astype(np.float32)


def test_synthetic_network_programs_match_the_expression_strings():
    """the compiler at the opcodes and the stack depth the shipped text never reaches: `interpret_programs` over the
    compiled 1025-gene synthetic network (deep chain and unary gene included) against Python's evaluation of the strings"""
    from oracle import hill_oracle
    from phoenix_amd.simulator import OPS, HillSystem
    names, exprs, info = synthetic_network(1025)
    sys_ = HillSystem(names, exprs, device="cpu")
    assert np.array_equal(sys_.is_input, info["is_input"])
    x = synthetic_states(1025, 4, info)
    assert np.any(x <= 0) and np.any(x > 1)
    want = hill_oracle.rhs(names, exprs, x, fact=hill_oracle.fAct0)
    got = hill_oracle.interpret_programs(sys_.code_host, sys_.consts_host, sys_.off_host, sys_.len_host, x)
    assert np.max(np.abs(got - want)) < 1e-12
    assert np.all(got[:, sys_.is_input] == 0)
    assert np.all(np.abs(want[:, info["deep"]] + x[:, info["deep"]]) > 1e-2)      # the 24-fold product is not negligible
    def ops_of(g):
        return sys_.code_host[sys_.off_host[g]: sys_.off_host[g] + sys_.len_host[g], 0].tolist()
    assert ops_of(info["unary"]).count(OPS["NEG"]) == 2 and ops_of(info["unary"]).count(OPS["DIV"]) == 2   # unary + emits nothing
    assert sys_.len_host[info["deep"]] == 127 and ops_of(info["deep"]).count(OPS["FACT"]) == CHAIN
    # where no state is negative the continuation of fAct is not used: the reference's own fAct gives the same bits
    xp = np.abs(x)
    assert np.array_equal(hill_oracle.rhs(names, exprs, xp), hill_oracle.rhs(names, exprs, xp, fact=hill_oracle.fAct0))
    # the row-by-row evaluation on Python floats that the trajectory references use is the same arithmetic
    rowwise = hill_oracle.compile_rhs(names, exprs, fact=hill_oracle.fAct0)(x, rowwise=True)
    assert np.max(np.abs(rowwise - want)) < 1e-14 and np.all(rowwise[:, sys_.is_input] == 0)


def test_a_stack_deeper_than_the_interpreter_holds_is_rejected():
    """MAX_STACK activations compile (the deep gene of every synthetic network), one more is a ValueError on the host"""
    from phoenix_amd import simulator as sim
    for L, ok in ((sim.MAX_STACK, True), (sim.MAX_STACK + 1, False)):
        names = ["R%d" % i for i in range(L)] + ["D"]
        edges = {(tf, "D"): {"from": tf, "weight": "1", "EC50": "0.3", "n": "2"} for tf in names[:L]}
        exprs = ["input gene"] * L + [sim.rate_expression("D", and_chain("D", names[:L], edges), edges)]
        assert compiled_depth(names, exprs[-1])[0] == L
        if ok:
            assert sim.HillSystem(names, exprs, device="cpu").len_host[L] == 127
        else:
            with pytest.raises(ValueError, match="deeper evaluation stack"):
                sim.HillSystem(names, exprs, device="cpu")
