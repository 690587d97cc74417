"""Host side of the pseudo-log-likelihood entries: the C ABI (exports, refusal without a context), a float64 numpy
restatement of the semantics checked against the CPU oracle's exact objective, the file writer, the argument parsing of the
compute_pseudo_log_likelihood sub-command (through a stand-in), and the argument checks of the classes.  No GPU needed;
tests/test_pseudo_likelihood.py imports the restatement from here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.dca_utilities import dca_utilities  # noqa: E402
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException  # noqa: E402

TOY_RNA = os.path.join(ROOT, "tests", "golden", "data", "toy_rna.fa")
ENTRIES = ("dca_plm_pseudo_likelihood", "dca_mf_pseudo_likelihood")


# ---------------------------------------------------------------- float64 numpy restatement (shared with the GPU tests)
def conditionals_ref(h, Jp, X):
    """h: L x q, Jp: pairs x q x q (pair order (0,1),(0,2)...; J_ij for i < j), X: n x L codes
    -> (pll[n], site[n, L], cond[n, L, q], umax[n]) in float64; umax = max |u_i(a)| per sequence.  The PLL is the
    ascending-i sum of the site values (np.cumsum adds in order)."""
    h = np.asarray(h, dtype=np.float64)
    L, q = h.shape
    iu, ju = np.triu_indices(L, 1)
    p = np.arange(iu.size)
    n = X.shape[0]
    cond = np.empty((n, L, q))
    umax = np.empty(n)
    for k in range(n):
        x = X[k].astype(np.int64)
        u = h.copy()
        np.add.at(u, iu, np.asarray(Jp[p, :, x[ju]], dtype=np.float64))      # J_ij(a, s_j), i < j
        np.add.at(u, ju, np.asarray(Jp[p, x[iu], :], dtype=np.float64))      # J_ji(s_i, a) = J_ij(a, s_i), j > i
        m = u.max(axis=1, keepdims=True)
        cond[k] = (u - m) - np.log(np.exp(u - m).sum(axis=1, keepdims=True))
        umax[k] = np.abs(u).max()
    site = cond[np.arange(n)[:, None], np.arange(L)[None, :], X.astype(np.int64)]
    pll = np.cumsum(site, axis=1)[:, -1] if L else np.zeros(n)
    return pll, site, cond, umax


def plm_model(x, L, q):
    x = np.asarray(x)
    return x[:L * q].reshape(L, q), x[L * q:].reshape(-1, q, q)


def mf_model(J, fields, L, q):
    """Dense -inv(C) (L(q-1) square) and fields (L x (q-1)) -> h, J with zero gap rows / columns."""
    qm = q - 1
    h = np.zeros((L, q))
    h[:, :qm] = fields
    J4 = np.asarray(J).reshape(L, qm, L, qm)
    iu, ju = np.triu_indices(L, 1)
    Jp = np.zeros((iu.size, q, q))
    Jp[:, :qm, :qm] = J4[iu, :, ju, :]
    return h, Jp


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, const uint8_t* X, int n, double* pll_out" in header
    assert '"pll"' in header


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    X = np.zeros((2, 4), dtype=np.uint8)
    out = np.zeros(2)
    for name in ENTRIES:
        assert getattr(lib, name)(None, X.ctypes.data, 2, out.ctypes.data, None, None) == _lib.DCA_ERR_ARG


# ---------------------------------------------------------------- the restatement against the oracle's exact objective
def test_restatement_matches_oracle_exact_objective(oracle_plm):
    """With no carry-over and zero penalties the oracle's fx is -sum_n w_n PLL(s_n): a second, independent statement of
    the identity the GPU test checks against dca_plm_gradient."""
    rng = np.random.default_rng(11)
    for L, q in ((6, 5), (9, 21)):
        X = rng.integers(0, q, size=(30, L), dtype=np.uint8)
        w = rng.uniform(0.2, 1.0, 30)
        x = rng.normal(0, 0.4, L * q + L * (L - 1) // 2 * q * q)
        fx, _g = oracle_plm.gradient(X, w, q, 0.0, 0.0, x, carry=False)
        h, Jp = plm_model(x, L, q)
        pll, site, cond, _umax = conditionals_ref(h, Jp, X)
        assert abs(fx + np.dot(w, pll)) <= 1e-11 * abs(fx)
        assert np.allclose(np.exp(cond).sum(axis=2), 1.0, rtol=0, atol=1e-13)


def test_restatement_agrees_with_energy_differences():
    """log P(s_i = a | s_-i) - log P(s_i = b | s_-i) = E(s with s_i = a) - E(s with s_i = b)"""
    rng = np.random.default_rng(3)
    L, q = 5, 4
    h = rng.normal(size=(L, q))
    Jp = rng.normal(size=(L * (L - 1) // 2, q, q))
    iu, ju = np.triu_indices(L, 1)

    def energy(s):
        return h[np.arange(L), s].sum() + Jp[np.arange(iu.size), s[iu], s[ju]].sum()
    s = rng.integers(0, q, L)
    _pll, _site, cond, _u = conditionals_ref(h, Jp, s[None, :].astype(np.uint8))
    for i in range(L):
        E = []
        for a in range(q):
            t = s.copy()
            t[i] = a
            E.append(energy(t))
        assert np.allclose(cond[0, i] - cond[0, i, 0], np.array(E) - E[0], atol=1e-12)


# ---------------------------------------------------------------- writer and command lines
def test_writer_layout(tmp_path):
    path = str(tmp_path / "pll.txt")
    dca_utilities.write_pseudo_log_likelihoods(path, np.array([-1.5, -2.0 / 3.0]), metadata=["# meta"], query_file="q.fa",
                                              weighted=-1.0 / 7.0)
    lines = open(path).read().splitlines()
    assert "# meta" in lines and "#\tQuery sequences: q.fa" in lines
    assert "#\tWeighted pseudo-log-likelihood per effective sequence: %.17g" % (-1.0 / 7.0) in lines
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert rows == [["1", "-1.5"], ["2", "%.17g" % (-2.0 / 3.0)]]
    assert float(rows[1][1]) == -2.0 / 3.0
    dca_utilities.write_pseudo_log_likelihoods(path, [], metadata=None, query_file=None, weighted=None)
    lines = open(path).read().splitlines()
    assert not any("Weighted" in ln for ln in lines) and not [ln for ln in lines if not ln.startswith("#")]


@pytest.mark.parametrize("main", ["plm", "mf"])
def test_subcommand_options(monkeypatch, main):
    mod, run = (plmdca_main, plmdca_main.run_plm_dca) if main == "plm" else (mfdca_main, mfdca_main.run_meanfield_dca)
    assert "compute_pseudo_log_likelihood" in _potts.POTTS_SUBCOMMANDS
    seen = {}
    monkeypatch.setattr(mod, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
    run(["compute_pseudo_log_likelihood", "rna", TOY_RNA, "--query_file", "q.fa"])
    assert seen["the_command"] == "compute_pseudo_log_likelihood" and seen["query_file"] == "q.fa"
    run(["compute_pseudo_log_likelihood", "rna", TOY_RNA])
    assert seen["query_file"] is None
    with pytest.raises(SystemExit):
        run(["compute_pseudo_log_likelihood", "rna", TOY_RNA, "--wildtype_file", "w.fa"])


class StandIn:
    """The calls run_subcommand makes for compute_pseudo_log_likelihood, recorded"""
    def __init__(self):
        self.calls = []

    def compute_sequence_pseudo_log_likelihoods(self, sequences=None):
        self.calls.append(("plls", sequences))
        return np.array([-1.5, -2.0 / 3.0, -4.0])

    def compute_pseudo_log_likelihood(self):
        self.calls.append(("weighted",))
        return -1.0 / 7.0


@pytest.mark.parametrize("query", [None, "q.fa"])
def test_subcommand_file(tmp_path, query):
    inst = StandIn()
    out = str(tmp_path / "out")
    path = _potts.run_subcommand(inst, "compute_pseudo_log_likelihood", "PLMDCA", TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA,
                                 0, PlmDCAException, query_file=query)
    assert os.path.basename(path) == "PLMDCA_pseudo_log_likelihoods_toy_rna.txt"
    assert inst.calls == ([("plls", None), ("weighted",)] if query is None else [("plls", "q.fa")])
    lines = open(path).read().splitlines()
    assert "# meta" in lines and "#\tQuery sequences: {}".format(query or TOY_RNA) in lines
    assert any("Weighted" in ln for ln in lines) == (query is None)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert [int(r[0]) for r in rows] == [1, 2, 3] and [float(r[1]) for r in rows] == [-1.5, -2.0 / 3.0, -4.0]


# ---------------------------------------------------------------- argument checks of the classes (before any device work)
def test_class_argument_checks():
    inst = PlmDCA(TOY_RNA, "rna")
    for bad in (1, "yes", None):
        with pytest.raises(PlmDCAException, match="per_site"):
            inst.compute_sequence_pseudo_log_likelihoods(per_site=bad)
    with pytest.raises(PlmDCAException, match="needs sequences"):
        inst.compute_conditional_log_probabilities(None)
    with pytest.raises(MeanFieldDCAException, match="per_site"):
        _potts.pll_flag(0, MeanFieldDCAException)
    assert _potts.single_query("ACGU", PlmDCAException) and not _potts.single_query(TOY_RNA, PlmDCAException)
    assert not _potts.single_query(["ACGU"], PlmDCAException)
    assert _potts.pseudo_log_likelihood([-1.0, -3.0], [1.0, 0.5], 1.5) == (-1.0 - 1.5) / 1.5


def test_class_methods_refuse_several_devices():
    inst = PlmDCA(TOY_RNA, "rna", devices=[0, 1])
    for call in (inst.compute_sequence_pseudo_log_likelihoods, inst.compute_pseudo_log_likelihood,
                 lambda: inst.compute_conditional_log_probabilities("ACGUACGUAC")):
        with pytest.raises(PlmDCAException, match="one GPU"):
            call()
