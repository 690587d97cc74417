"""Host side of the three-site connected correlations (dca_three_site_values, dca_three_site_scan): the
exported symbols and their declarations, NULL contexts, the Python argument checks, the ArDCA element mapping and the numpy
brute force (tests/three_site_reference.py) that tests/test_three_site.py holds the GPU against.  No GPU needed."""
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT, data_file
from three_site_reference import all_elements, brute_force, flat, quantised_weights, tile_side, top_elements
from pydca_amd import _compare, _lib, ardca_main, mfdca_main, plmdca_main
from pydca_amd.ardca.ardca import ArDCA, ArDCAException
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

TOY_RNA = data_file("toy_rna.fa")


# ---------------------------------------------------------------- 1-3: the C ABI as far as the host reaches
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = " ".join(open(os.path.join(ROOT, "include", "dca_hip.h")).read().split())
    for name in ("dca_three_site_values", "dca_three_site_scan"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert ("int dca_three_site_values(dca_ctx* ctx, const uint8_t* Q, int nq, const int32_t* elements, int T, uint64_t* count_out, "
            "uint64_t* denom_out, double* f3_out, double* c3_out);") in header
    assert ("int dca_three_site_scan(dca_ctx* ctx, const uint8_t* Q, int nq, int K, int skip_state, int32_t* elements_out, "
            "double* c3_out, double* f3_out, int* found);") in header
    assert '"three_site_scan"' in header and '"three_site_values"' in header and "2^40" in header


def test_entries_refuse_a_null_context():
    import ctypes as C
    lib = _lib.lib()
    el = np.array([[0, 1, 2, 0, 0, 0]], dtype=np.int32)
    c = np.zeros(1)
    found = C.c_int(0)
    assert lib.dca_three_site_values(None, None, 0, el.ctypes.data, 1, None, None, None, c.ctypes.data) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()
    out = np.zeros((1, 6), dtype=np.int32)
    assert lib.dca_three_site_scan(None, None, 0, 1, -1, out.ctypes.data, c.ctypes.data, None, C.byref(found)) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()


@pytest.mark.parametrize("cls, exc", [(PlmDCA, PlmDCAException), (ArDCA, ArDCAException)])
def test_class_argument_checks(cls, exc):
    inst = cls(TOY_RNA, "rna")
    for bad in (0, -3):
        with pytest.raises(exc, match="num_top must be >= 1"):
            inst.compute_top_three_site_correlations(num_top=bad)
    for bad in (2.5, "7", None, True):
        with pytest.raises(exc, match="num_top must be an integer"):
            inst.compute_top_three_site_correlations(num_top=bad)
    for bad in (1, "yes", None):
        with pytest.raises(exc, match="include_gaps"):
            inst.compute_top_three_site_correlations(5, include_gaps=bad)
        with pytest.raises(exc, match="three_site_include_gaps"):
            inst.compare_with_alignment(["ACGUACGUAC"], three_site=3, three_site_include_gaps=bad)
    with pytest.raises(exc, match="three_site must be >= 0"):
        inst.compare_with_alignment(["ACGUACGUAC"], three_site=-1)
    with pytest.raises(exc, match="three_site must be an integer"):
        inst.compare_with_alignment(["ACGUACGUAC"], three_site=1.0)
    good = [0, 1, 2, 0, 0, 0]
    for bad, what in (([good[:5]], "shape"), (good, "shape"), (np.zeros((0, 6), dtype=np.int32), "at least one row"),
                      (np.array([good], dtype=np.float64), "integer array"), ([[1, 1, 2, 0, 0, 0]], "0 <= i < j < k < 10"),
                      ([[2, 1, 3, 0, 0, 0]], "0 <= i < j < k < 10"), ([[0, 1, 10, 0, 0, 0]], "0 <= i < j < k < 10"),
                      ([[-1, 1, 2, 0, 0, 0]], "0 <= i < j < k < 10"), ([good, [0, 1, 2, 0, 5, 0]], "element 1 names the states"),
                      ([[0, 1, 2, -1, 0, 0]], "states are 0 .. 4")):
        with pytest.raises(exc, match=what):
            inst.compute_three_site_correlations(bad)


def test_methods_and_options_on_every_class_and_command_line(monkeypatch):
    for cls in (PlmDCA, MeanFieldDCA, ArDCA):
        assert issubclass(cls, _compare.SequenceComparison)
        for name in ("compute_top_three_site_correlations", "compute_three_site_correlations"):
            assert getattr(cls, name) is getattr(_compare.SequenceComparison, name)
    for mod, run in ((plmdca_main, plmdca_main.run_plm_dca), (mfdca_main, mfdca_main.run_meanfield_dca), (ardca_main, ardca_main.run_ardca)):
        seen = {}
        monkeypatch.setattr(mod, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
        run(["compare_sequences", "rna", TOY_RNA, "--query_file", "s.fa", "--three_site", "500", "--three_site_no_gaps"])
        assert seen["three_site"] == 500 and seen["three_site_no_gaps"] is True
        run(["compare_sequences", "rna", TOY_RNA, "--query_file", "s.fa"])
        assert seen["three_site"] == 0 and seen["three_site_no_gaps"] is False


class StandIn:
    sequences_len = 4

    def __init__(self):
        self.kw = None

    def compare_with_alignment(self, sequences, **kw):
        self.kw = kw
        out = {"pearson_cij": 0.5, "num_sequences": 2}
        if kw.get("three_site"):
            out.update(pearson_cijk=0.25, slope_cijk=0.5, max_abs_diff_cijk=0.125, three_site_terms=kw["three_site"])
        return out

    def compute_distances_to_alignment(self, sequences, return_index=False, return_histogram=False):
        return np.array([1, 4], dtype=np.int32), np.array([7, 0], dtype=np.int32), np.array([0, 1, 0, 0, 1], dtype=np.uint64)

    def compute_alignment_self_distances(self, return_index=False, return_histogram=False):
        return np.array([2], dtype=np.int32), np.array([0, 0, 6, 0, 0], dtype=np.uint64)


def test_comparison_file_gains_four_lines_only_with_the_option(tmp_path):
    inst = StandIn()
    plain = _compare.run_compare(inst, "PLMDCA", TOY_RNA, str(tmp_path / "a"), ["# meta"], "q.fa", PlmDCAException)
    assert inst.kw == {}                                              # the call of today, so the file of today
    with3 = _compare.run_compare(inst, "PLMDCA", TOY_RNA, str(tmp_path / "b"), ["# meta"], "q.fa", PlmDCAException, three_site=7,
                                 three_site_include_gaps=False)
    assert inst.kw == {"three_site": 7, "three_site_include_gaps": False}
    a, b = open(plain).read().splitlines(), open(with3).read().splitlines()
    assert sorted(set(b) - set(a)) == ["#\tmax_abs_diff_cijk: 0.125", "#\tpearson_cijk: 0.25", "#\tslope_cijk: 0.5", "#\tthree_site_terms: 7"]
    assert [ln for ln in b if ln in a] == a


# ---------------------------------------------------------------- 4: the ArDCA element mapping
def test_element_mapping_round_trips_under_random_permutations():
    rng = np.random.default_rng(11)
    for L, q in ((3, 5), (8, 21), (40, 4)):
        el = all_elements(L, q) if L <= 3 else None
        if el is None:
            sites = np.sort(np.stack([rng.choice(L, size=3, replace=False) for _ in range(500)]), axis=1)
            el = np.concatenate([sites, rng.integers(0, q, size=(500, 3))], axis=1).astype(np.int32)
        for _ in range(5):
            order = rng.permutation(L)
            ctx_el = _compare.elements_to_order(el, order)
            assert ctx_el.dtype == np.int32 and ctx_el.shape == el.shape
            assert (ctx_el[:, 0] < ctx_el[:, 1]).all() and (ctx_el[:, 1] < ctx_el[:, 2]).all()
            back = _compare.elements_from_order(ctx_el, order)
            assert np.array_equal(back, el)
            assert np.array_equal(_compare.elements_to_order(_compare.elements_from_order(el, order), order), el)
            # every state follows its site: (file site, state) pairs are the same set on both sides
            for r, c in zip(el[:50], ctx_el[:50]):
                assert {(int(r[s]), int(r[3 + s])) for s in range(3)} == {(int(order[c[s]]), int(c[3 + s])) for s in range(3)}
        assert np.array_equal(_compare.elements_from_order(el, np.arange(L)), el)


def test_element_mapping_matches_a_permuted_alignment():
    rng = np.random.default_rng(12)
    L, q = 5, 3
    X = rng.integers(0, q, size=(30, L), dtype=np.uint8)
    order = np.array([3, 0, 4, 1, 2])
    wq = np.ones(30, dtype=np.uint64)
    ref, refp = brute_force(X, wq, q), brute_force(X[:, order], wq, q)
    el_ctx = all_elements(L, q)
    el_file = _compare.elements_from_order(el_ctx, order)
    cp = flat(refp, "c3", L)
    for r, v in zip(el_file, cp):
        assert abs(ref["c3"][tuple(r[:3])][tuple(r[3:])] - v) <= 4e-15       # the same element; the order of the three products differs


# ---------------------------------------------------------------- 5: the brute force on its own
def test_tile_rule():
    assert [tile_side(q) for q in (2, 5, 10, 11, 21, 22, 32)] == [8, 8, 8, 4, 4, 2, 2]


def test_brute_force_hand_example():
    X = np.array([[0, 0, 0], [0, 0, 1], [1, 1, 1], [1, 0, 1]], dtype=np.uint8)
    ref = brute_force(X, np.ones(4, dtype=np.uint64), 2)
    assert ref["denom"] == 4 and ref["n3"][0, 1, 2].dtype == np.uint64
    assert ref["n3"][0, 1, 2].tolist() == [[[1, 1], [0, 0]], [[0, 1], [0, 1]]]
    # c_012(0,0,0) = 1/4 - (2/4)(1/4) - (1/4)(3/4) - (1/4)(2/4) + 2 (2/4)(3/4)(1/4)
    assert ref["c3"][0, 1, 2][0, 0, 0] == 0.25 - 0.5 * 0.25 - 0.25 * 0.75 - 0.25 * 0.5 + 2.0 * 0.5 * 0.75 * 0.25
    el, c, f = top_elements(ref, 3, 2, 3)
    assert el.shape == (3, 6) and np.all(np.abs(c[:-1]) >= np.abs(c[1:])) and f[0] == ref["f3"][0, 1, 2][tuple(el[0, 3:])]


@pytest.mark.parametrize("q, L, N", [(5, 6, 63), (21, 4, 40)])
def test_brute_force_blocks_sum_to_zero_and_marginals_agree(q, L, N):
    rng = np.random.default_rng(100 * q + L)
    X = rng.integers(0, q, size=(N, L), dtype=np.uint8)
    w = 1.0 / rng.integers(1, 9, size=N)
    for wq in (np.ones(N, dtype=np.uint64), quantised_weights(w)):
        ref = brute_force(X, wq, q)
        assert ref["denom"] == int(sum(int(v) for v in wq))
        for t in itertools.combinations(range(L), 3):
            i, j, k = t
            n = ref["n3"][t]
            assert n.dtype == np.uint64 and int(n.sum(dtype=np.uint64)) == ref["denom"]
            assert np.array_equal(n.sum(axis=2, dtype=np.uint64), ref["n2"][i, j]) and np.array_equal(n.sum(axis=0, dtype=np.uint64), ref["n2"][j, k])
            assert np.array_equal(n.sum(axis=(1, 2), dtype=np.uint64), ref["n1"][i])
            for axis in range(3):
                assert np.abs(ref["c3"][t].sum(axis=axis)).max() <= 1e-13
    # the quantisation itself: llrint(w 2^40), exact for weights 1 / 2^k
    assert quantised_weights([1.0, 0.5, 1.0 / 3.0]).tolist() == [2 ** 40, 2 ** 39, 366503875925]
    el = all_elements(L, q, skip_state=q - 1)
    assert el.shape == (L * (L - 1) * (L - 2) // 6 * (q - 1) ** 3, 6) and not (el[:, 3:] == q - 1).any()
