"""Host side of the sequence-set comparison (dca_hamming_nearest, dca_sequence_statistics): the C ABI (exports, declarations,
refusals), integer / float64 numpy restatements of the semantics -- checked on a hand-computed 3 x 4 example and, for the
alignment side, against the CPU oracle's weighted frequencies --, the file writer, the parsing of the compare_sequences
sub-command (through a stand-in) and the argument checks of the classes.  No GPU needed; tests/test_sequence_comparison.py
imports the restatements from here."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _compare, _lib, _potts, ardca_main, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.ardca.ardca import ArDCA, ArDCAException  # noqa: E402
from pydca_amd.dca_utilities import dca_utilities  # noqa: E402
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException  # noqa: E402

TOY_RNA = os.path.join(ROOT, "tests", "golden", "data", "toy_rna.fa")
ENTRIES = ("dca_hamming_nearest", "dca_sequence_statistics", "dca_alignment_statistics")


# ---------------------------------------------------------------- numpy restatements (shared with the GPU tests)
def nearest_ref(Q, R, skip_same=False):
    """Q: nq x L, R: nr x L codes -> (dist int32[nq], index int32[nq], hist uint64[L + 1]) of dca_hamming_nearest: minimum over the
    compared rows m (all, or m != k with skip_same), the smallest m on ties, -1 / -1 without partner; hist over compared pairs."""
    Q, R = np.asarray(Q, dtype=np.uint8), np.asarray(R, dtype=np.uint8)
    nq, L = Q.shape
    nr = R.shape[0]
    dist = np.full(nq, -1, dtype=np.int32)
    index = np.full(nq, -1, dtype=np.int32)
    hist = np.zeros(L + 1, dtype=np.uint64)
    step = max(1, int(4e7 // max(1, nr * L)))
    for s in range(0, nq, step):
        D = (Q[s:s + step, None, :] != R[None, :, :]).sum(axis=2).astype(np.int64)          # rows x nr
        keep = np.ones(D.shape, dtype=bool)
        if skip_same:
            k = np.arange(s, s + D.shape[0])
            inside = k < nr
            keep[np.nonzero(inside)[0], k[inside]] = False
        hist += np.bincount(D[keep], minlength=L + 1).astype(np.uint64)
        masked = np.where(keep, D, L + 1)
        m = masked.argmin(axis=1)                    # the first (smallest) index of the minimum
        d = masked[np.arange(D.shape[0]), m]
        has = d <= L
        dist[s:s + step] = np.where(has, d, -1)
        index[s:s + step] = np.where(has, m, -1)
    return dist, index, hist


def set_frequencies_ref(Q, q, w=None):
    """One- and two-site frequencies of the rows of Q (all q states, pair order): w None -> count / n, one IEEE division of
    exact integers; else sum_n w_n [..] / sum_n w_n in float64.  -> (fi L x q, fij pairs x q x q)"""
    Q = np.asarray(Q)
    n, L = Q.shape
    iu, ju = np.triu_indices(L, 1)
    if w is None:
        oh = np.zeros((n, L, q), dtype=np.int64)
        oh[np.arange(n)[:, None], np.arange(L)[None, :], Q.astype(np.int64)] = 1
        ci = oh.sum(axis=0)
        cij = np.einsum("nia,njb->ijab", oh, oh)[iu, ju]
        return ci.astype(np.float64) / np.float64(n), cij.astype(np.float64) / np.float64(n)
    w = np.asarray(w, dtype=np.float64)
    oh = np.zeros((n, L, q), dtype=np.float64)
    oh[np.arange(n)[:, None], np.arange(L)[None, :], Q.astype(np.int64)] = 1.0
    meff = w.sum()
    fi = np.einsum("n,nia->ia", w, oh) / meff
    fij = np.einsum("nia,njb->ijab", oh * w[:, None, None], oh)[iu, ju] / meff
    return fi, fij


def compare_ref(xi, xij, yi, yij):
    """The dca_set_comparison of alignment-side (x) and set-side (y) frequencies with exactly rounded sums (math.fsum) of the
    double terms the device forms: per quantity k (0 f_i, 1 f_ij, 2 c_ij) sxx, syy, sxy, max_abs_diff, pearson, slope, terms and
    abs_* = the sums of |term| (what the error bound of a double sum in any order is proportional to)."""
    xi, xij, yi, yij = (np.asarray(v, dtype=np.float64) for v in (xi, xij, yi, yij))
    L, q = xi.shape
    iu, ju = np.triu_indices(L, 1)
    cx = xij - xi[iu][:, :, None] * xi[ju][:, None, :]
    cy = yij - yi[iu][:, :, None] * yi[ju][:, None, :]
    mu1, mu2 = 1.0 / np.float64(q), 1.0 / np.float64(q * q)
    out = {k: np.zeros(3) for k in ("sxx", "syy", "sxy", "abs_sxx", "abs_syy", "abs_sxy", "max_abs_diff", "pearson", "slope", "terms")}
    for k, (dx, dy, diff) in enumerate(((xi - mu1, yi - mu1, xi - yi), (xij - mu2, yij - mu2, xij - yij), (cx, cy, cx - cy))):
        dx, dy = dx.reshape(-1), dy.reshape(-1)
        for name, t in (("sxx", dx * dx), ("syy", dy * dy), ("sxy", dx * dy)):
            out[name][k] = math.fsum(t)
            out["abs_" + name][k] = math.fsum(np.abs(t))
        out["max_abs_diff"][k] = np.abs(diff).max() if diff.size else 0.0
        vv = out["sxx"][k] * out["syy"][k]
        out["pearson"][k] = out["sxy"][k] / math.sqrt(vv) if vv > 0.0 else 0.0
        out["slope"][k] = out["sxy"][k] / out["sxx"][k] if out["sxx"][k] > 0.0 else 0.0
        out["terms"][k] = dx.size
    return out


def set_statistics_ref(Q, X, w, q):
    """Set Q against alignment X with weights w -> (fi, fij of the set, fi, fij of the alignment, compare_ref of the two)"""
    yi, yij = set_frequencies_ref(Q, q)
    xi, xij = set_frequencies_ref(X, q, w)
    return yi, yij, xi, xij, compare_ref(xi, xij, yi, yij)


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, " in header
    assert "int dca_hamming_nearest(dca_ctx* ctx, const uint8_t* Q, int nq, const uint8_t* R, int nr, int skip_same_index," in header
    assert "int32_t* dist_out, int32_t* index_out, uint64_t* hist_out);" in header
    assert ("int dca_sequence_statistics(dca_ctx* ctx, const uint8_t* Q, int nq, double* fi_out, double* fij_out, "
            "dca_set_comparison* cmp_out);") in header
    assert "} dca_set_comparison;" in header and '"hamming"' in header
    assert C.sizeof(_lib.SetComparison) == 21 * 8


def test_entries_refuse_a_null_context():
    """DCA_ERR_ARG with the message in dca_last_error(); the NULL outputs of a live context are refused in the GPU tests."""
    lib = _lib.lib()
    Q = np.zeros((2, 4), dtype=np.uint8)
    d = np.zeros(2, dtype=np.int32)
    fi = np.zeros((4, 5))
    cmp_ = _lib.SetComparison()
    assert lib.dca_hamming_nearest(None, Q.ctypes.data, 2, Q.ctypes.data, 2, 0, d.ctypes.data, None, None) == _lib.DCA_ERR_ARG
    assert lib.dca_sequence_statistics(None, Q.ctypes.data, 2, fi.ctypes.data, None, C.byref(cmp_)) == _lib.DCA_ERR_ARG
    assert lib.dca_alignment_statistics(None, fi.ctypes.data, None) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()


# ---------------------------------------------------------------- the restatements
def test_nearest_ref_hand_example():
    Q = np.array([[0, 1, 0, 1], [0, 1, 1, 1], [1, 1, 0, 0]], dtype=np.uint8)
    R = np.array([[0, 1, 0, 1], [1, 0, 1, 0]], dtype=np.uint8)
    # distances: Q0 (0, 4), Q1 (1, 3), Q2 (2, 2) -> a tie that goes to the smaller index
    d, m, h = nearest_ref(Q, R)
    assert d.tolist() == [0, 1, 2] and m.tolist() == [0, 0, 0] and h.tolist() == [1, 1, 2, 1, 1]
    # skipping k == m: Q0 sees R1 only, Q1 sees R0 only, Q2 (no row 2 in R) sees both
    d, m, h = nearest_ref(Q, R, skip_same=True)
    assert d.tolist() == [4, 1, 2] and m.tolist() == [1, 0, 0] and h.tolist() == [0, 1, 2, 0, 1] and h.sum() == 3 * 2 - 2
    # the set against itself: d(Q0, Q1) = 1, d(Q0, Q2) = 2, d(Q1, Q2) = 3
    d, m, h = nearest_ref(Q, Q, skip_same=True)
    assert d.tolist() == [1, 1, 2] and m.tolist() == [1, 0, 0] and h.tolist() == [0, 2, 2, 2, 0]
    d, m, h = nearest_ref(Q[:1], Q[:1], skip_same=True)
    assert d.tolist() == [-1] and m.tolist() == [-1] and h.sum() == 0


def test_set_statistics_ref_hand_example():
    Q = np.array([[0, 1, 0, 1], [0, 1, 1, 1], [1, 1, 0, 0]], dtype=np.uint8)
    fi, fij = set_frequencies_ref(Q, 2)
    third = np.float64(1) / np.float64(3)
    two = np.float64(2) / np.float64(3)
    assert np.array_equal(fi, np.array([[two, third], [0.0, 1.0], [two, third], [third, two]]))
    assert fij.shape == (6, 2, 2)
    assert np.array_equal(fij[1], np.array([[third, third], [third, 0.0]]))        # pair (0, 2)
    assert np.array_equal(fij[5], np.array([[third, third], [0.0, third]]))        # pair (2, 3): rows (0, 1), (1, 1), (0, 0)
    # uniform weights are the unweighted frequencies up to the rounding of the weighted sums
    gi, gij = set_frequencies_ref(Q, 2, np.ones(3))
    assert np.allclose(gi, fi, rtol=0, atol=1e-15) and np.allclose(gij, fij, rtol=0, atol=1e-15)
    # a set compared with itself: Pearson and slope 1, no deviation; c_01(1, 1) = 1/3 - 1/3 * 1 = 0
    c = compare_ref(fi, fij, fi, fij)
    assert np.array_equal(c["pearson"], np.ones(3)) and np.array_equal(c["slope"], np.ones(3))
    assert np.array_equal(c["max_abs_diff"], np.zeros(3)) and c["terms"].tolist() == [8, 24, 24]
    # f_i centred with 1 / q = 1/2: two sites (1/6)^2 * 2, one site (1/2)^2 * 2, one more (1/6)^2 * 2
    assert abs(c["sxx"][0] - (6 / 36 + 0.5)) < 1e-15
    # against other frequencies: x = y / 2 + 1/4 centres to half of y's deviations -> slope of y on x is 2, Pearson 1
    c = compare_ref(fi / 2 + 0.25, fij, fi, fij)
    assert abs(c["slope"][0] - 2.0) < 1e-14 and abs(c["pearson"][0] - 1.0) < 1e-14
    assert c["max_abs_diff"][0] == 0.25                      # |x - y| = |1/4 - y/2|, largest at site 1 where y is 0 and 1


def test_alignment_side_matches_the_oracle(oracle_mf):
    seqs = oracle_mf.read_fasta(TOY_RNA)
    X1 = oracle_mf.letter2int(seqs, "rna")              # 1-based states, gap = q
    w = oracle_mf.compute_sequences_weight(X1, 0.8)
    fi_o = oracle_mf.compute_single_site_freqs(X1, 5, w)
    fij_o = oracle_mf.compute_pair_site_freqs(X1, 5, w)
    fi, fij = set_frequencies_ref((X1 - 1).astype(np.uint8), 5, w)
    assert np.allclose(fi, fi_o, rtol=0, atol=1e-13)
    assert np.allclose(fij[:, :4, :4], fij_o, rtol=0, atol=1e-13)
    assert np.allclose(fi.sum(axis=1), 1.0, atol=1e-13) and np.allclose(fij.sum(axis=(1, 2)), 1.0, atol=1e-13)


def test_pairs_to_order_undoes_a_column_permutation():
    rng = np.random.default_rng(4)
    Q = rng.integers(0, 5, size=(40, 6), dtype=np.uint8)
    order = rng.permutation(6)
    _fi, fij = set_frequencies_ref(Q, 5)
    _gi, gij = set_frequencies_ref(Q[:, order], 5)
    assert np.array_equal(_compare.pairs_to_order(gij, order), fij)
    assert _compare.distance_summary(np.array([3, -1, 1, 2])) == (2.0, 2.0, 1.0)
    assert all(math.isnan(v) for v in _compare.distance_summary(np.array([-1])))


# ---------------------------------------------------------------- writer and command lines
def test_writer_layout(tmp_path):
    path = str(tmp_path / "cmp.txt")
    summary = {"pearson_fi": 1.0 / 3.0, "num_sequences": 2, "nearest_distance": np.array([0, 3], dtype=np.int32)}
    dca_utilities.write_sequence_comparison(path, summary, [0, 3], [5, 1], np.array([1, 0, 0, 7], dtype=np.uint64),
                                            np.array([0, 0, 2, 4], dtype=np.uint64), 3, metadata=["# meta"], query_file="q.fa")
    lines = open(path).read().splitlines()
    assert "# meta" in lines and "#\tQuery sequences: q.fa" in lines
    assert "#\tpearson_fi: %.17g" % (1.0 / 3.0) in lines and "#\tnum_sequences: 2" in lines
    assert not any("nearest_distance" in ln for ln in lines)                        # arrays are not header material
    assert [ln for ln in lines if ln.startswith("#\tdistance ")] == ["#\tdistance 0: 1 0", "#\tdistance 2: 0 2", "#\tdistance 3: 7 4"]
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert rows == [["1", "0", "5", "1"], ["2", "3", "1", "0"]]


@pytest.mark.parametrize("main", ["plm", "mf", "ar"])
def test_subcommand_options(monkeypatch, main):
    mod, run = {"plm": (plmdca_main, plmdca_main.run_plm_dca), "mf": (mfdca_main, mfdca_main.run_meanfield_dca),
                "ar": (ardca_main, ardca_main.run_ardca)}[main]
    assert "compare_sequences" in _potts.POTTS_SUBCOMMANDS and "compare_sequences" in ardca_main.ARDCA_SUBCOMMANDS
    seen = {}
    monkeypatch.setattr(mod, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
    run(["compare_sequences", "rna", TOY_RNA, "--query_file", "samples.fa", "--output_dir", "out"])
    assert seen["the_command"] == "compare_sequences" and seen["query_file"] == "samples.fa" and seen["output_dir"] == "out"
    with pytest.raises(SystemExit):
        run(["compare_sequences", "rna", TOY_RNA])                                    # --query_file is required


class StandIn:
    """The calls run_compare makes, recorded; no fitting method exists, so none can be called"""
    sequences_len = 4

    def __init__(self):
        self.calls = []

    def compare_with_alignment(self, sequences, return_frequencies=False):
        self.calls.append(("compare", sequences))
        return {"pearson_cij": 0.5, "num_sequences": 2, "nearest_distance": np.array([1, 4], dtype=np.int32)}

    def compute_distances_to_alignment(self, sequences, return_index=False, return_histogram=False):
        self.calls.append(("distances", sequences, return_index, return_histogram))
        return np.array([1, 4], dtype=np.int32), np.array([7, 0], dtype=np.int32), np.array([0, 1, 0, 0, 1], dtype=np.uint64)

    def compute_alignment_self_distances(self, return_index=False, return_histogram=False):
        self.calls.append(("self", return_index, return_histogram))
        return np.array([2], dtype=np.int32), np.array([0, 0, 6, 0, 0], dtype=np.uint64)


@pytest.mark.parametrize("prefix", ["PLMDCA", "MFDCA"])
def test_subcommand_file(tmp_path, prefix):
    inst = StandIn()
    out = str(tmp_path / "out")
    path = _potts.run_subcommand(inst, "compare_sequences", prefix, TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA, 0,
                                 PlmDCAException, query_file="q.fa")
    assert os.path.basename(path) == prefix + "_sequence_comparison_toy_rna.txt"
    assert inst.calls == [("compare", "q.fa"), ("distances", "q.fa", True, True), ("self", False, True)]
    lines = open(path).read().splitlines()
    assert "#\tpearson_cij: 0.5" in lines and "#\tdistance 2: 0 6" in lines and "#\tdistance 4: 1 0" in lines
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert rows == [["1", "1", "7", "0.75"], ["2", "4", "0", "0"]]
    with pytest.raises(PlmDCAException, match="query_file"):
        _potts.run_subcommand(inst, "compare_sequences", prefix, TOY_RNA, out, [], _lib.DCA_BIOMOLECULE_RNA, 0, PlmDCAException)


# ---------------------------------------------------------------- argument checks of the classes (before any device work)
@pytest.mark.parametrize("cls, exc", [(PlmDCA, PlmDCAException), (ArDCA, ArDCAException)])
def test_class_argument_checks(cls, exc):
    inst = cls(TOY_RNA, "rna")
    for bad in (1, "yes", None):
        with pytest.raises(exc, match="return_index"):
            inst.compute_distances_to_alignment(["ACGUACGUAC"], return_index=bad)
        with pytest.raises(exc, match="return_histogram"):
            inst.compute_alignment_self_distances(return_histogram=bad)
        with pytest.raises(exc, match="return_frequencies"):
            inst.compare_with_alignment(["ACGUACGUAC"], return_frequencies=bad)
    with pytest.raises(exc, match="needs sequences"):
        inst.compute_distances_to_alignment(None)
    with pytest.raises(exc, match="needs at least one"):
        inst.compute_set_diversity([])
    with pytest.raises(exc, match="query record 2 is rejected: its length"):
        inst.compare_with_alignment(["ACGUACGUAC", "ACGU"])
    with pytest.raises(exc, match="query record 1 is rejected: it holds a character"):
        inst.compute_set_diversity(["ACGUACGUA!"])


def test_mixin_is_shared_by_the_three_classes():
    for cls in (PlmDCA, MeanFieldDCA, ArDCA):
        assert issubclass(cls, _compare.SequenceComparison)
        for name in ("compute_distances_to_alignment", "compute_alignment_self_distances", "compute_set_diversity",
                     "compare_with_alignment"):
            assert getattr(cls, name) is getattr(_compare.SequenceComparison, name)
    assert MeanFieldDCA._compare_exc is MeanFieldDCAException and MeanFieldDCA._compare_table == 1


def test_class_methods_refuse_several_devices():
    inst = PlmDCA(TOY_RNA, "rna", devices=[0, 1])
    for call in (lambda: inst.compute_distances_to_alignment(["ACGUACGUAC"]), inst.compute_alignment_self_distances,
                 lambda: inst.compute_set_diversity(["ACGUACGUAC"]), lambda: inst.compare_with_alignment(["ACGUACGUAC"])):
        with pytest.raises(PlmDCAException, match="one GPU"):
            call()
