"""Three-site connected correlations on the GPU (dca_three_site_values, dca_three_site_scan, the class methods and the command
line) against the numpy brute force of tests/three_site_reference.py.  Counts, denominators and f3 are compared exactly, c3
within 4e-15 absolute (nine double operations on magnitudes <= 2 bound the error by 2e-15); the scan's elements and their order
are compared exactly, which also needs c3 bit-equal wherever two elements tie or nearly tie.  Shapes: one triple, one tile
and one site more or less than whole tiles (TB = 4 at q = 21, 8 at q = 5), N = 1, 63, 257, a site with a single state."""
import itertools
import os

import numpy as np
import pytest

from conftest import data_file
from three_site_reference import all_elements, brute_force, flat, quantised_weights, tile_side, top_elements
from pydca_amd import _lib, plmdca_main
from pydca_amd.ardca.ardca import ArDCA
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
from pydca_amd.plmdca.plmdca import PlmDCA

pytestmark = pytest.mark.gpu

TODAYS_KEYS = {"num_sequences", "nearest_distance", "nearest_distance_mean", "nearest_distance_median", "nearest_distance_min",
               "fraction_identical", "alignment_self_distance_mean", "alignment_self_distance_median", "alignment_self_distance_min"} | {
                   "{}_{}".format(n, w) for n in ("pearson", "slope", "max_abs_diff") for w in ("fi", "fij", "cij")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_alignment(rng, N, L, q, single_state_site=None):
    prof = rng.dirichlet(np.full(q, 0.4), size=L)
    X = np.stack([rng.choice(q, size=N, p=prof[i]) for i in range(L)], axis=1).astype(np.uint8)
    if L >= 3:
        X[:, L - 1] = np.where(rng.random(N) < 0.7, X[:, 0], X[:, L - 1])        # something to find
    if single_state_site is not None:
        X[:, single_state_site] = 2
    return np.ascontiguousarray(X)


def check_against_brute_force(ctx, X, q, Q, wq, what, Ks=(1, 50, None), skips=(-1,)):
    """every element's count / denominator / f3 / c3 and the scans of the alignment (Q None) or of the set Q"""
    rows = X if Q is None else Q
    L = X.shape[1]
    ref = brute_force(rows, wq, q)
    el = all_elements(L, q)
    count, denom, f3, c3 = ctx.three_site_values(el, Q)
    assert count.dtype == np.uint64 and np.array_equal(count, flat(ref, "n3", L)), what
    assert denom == ref["denom"], what
    assert np.array_equal(bits(f3), bits(count.astype(np.float64) / np.float64(denom))), what
    rc = flat(ref, "c3", L)
    err = np.abs(c3 - rc).max()
    print(what, "values: T", el.shape[0], "max |c3 - brute force|", err, "bit-equal", np.array_equal(bits(c3), bits(rc)))
    assert err <= 4e-15, what
    for skip in skips:
        eligible = el.shape[0] if skip < 0 else int((~(el[:, 3:] == skip).any(axis=1)).sum())
        for K in Ks:
            K = eligible + 7 if K is None else K
            gel, gc, gf = ctx.three_site_scan(K, Q, skip)
            rel, rc3, rf3 = top_elements(ref, L, q, K, skip)
            assert gel.shape[0] == min(K, eligible), (what, K, skip)                  # found
            assert np.array_equal(gel, rel), (what, K, skip)
            assert np.array_equal(bits(gc), bits(rc3)) and np.array_equal(bits(gf), bits(rf3)), (what, K, skip)
    return ref, count


# ---------------------------------------------------------------- 1 + 3: values and scans at the edge shapes
@pytest.mark.parametrize("q, L, N", [(21, 3, 63), (21, 4, 1), (21, 4, 257), (21, 5, 63), (21, 7, 63), (21, 9, 63),
                                     (5, 3, 1), (5, 7, 257), (5, 9, 63), (5, 15, 63), (5, 17, 257), (32, 5, 63)])
def test_synthetic_alignments_and_sets(q, L, N):
    TB = tile_side(q)
    assert L <= 4 or any(L == TB * m + s for m in (1, 2) for s in (1, -1)) or q == 32
    rng = np.random.default_rng(1000 * q + 10 * L + N)
    X = random_alignment(rng, N, L, q, single_state_site=1 if L >= 4 else None)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    check_against_brute_force(ctx, X, q, None, quantised_weights(w), ("alignment", q, L, N))
    ctx.set_weights(np.ones(N))
    check_against_brute_force(ctx, X, q, None, np.full(N, 2 ** 40, dtype=np.uint64), ("uniform", q, L, N), Ks=(50,))
    Q = random_alignment(rng, 70, L, q)
    check_against_brute_force(ctx, X, q, Q, np.ones(70, dtype=np.uint64), ("set", q, L, N), skips=(-1, q - 1))
    assert np.array_equal(ctx.weights(), np.ones(N))                        # nothing of the context changed
    ctx.close()


@pytest.mark.parametrize("name, bio, q, L", [("toy_protein.fa", _lib.DCA_BIOMOLECULE_PROTEIN, 21, 8), ("toy_rna.fa", _lib.DCA_BIOMOLECULE_RNA, 5, 10)])
def test_toy_alignments_all_elements(name, bio, q, L):
    X = _lib.read_msa(data_file(name), bio, L)[0]
    N = X.shape[0]
    rng = np.random.default_rng(q)
    Q = X[rng.integers(0, N, size=300)].copy()
    flip = rng.random(Q.shape) < 0.2
    Q[flip] = rng.integers(0, q, size=int(flip.sum()), dtype=np.uint8)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    meff = float(w.sum())
    ref, count = check_against_brute_force(ctx, X, q, None, quantised_weights(w), name, skips=(-1, q - 1))
    # 2. the alignment's implied one- and two-site frequencies against dca_alignment_statistics: the quantisation bound
    xi, xij = ctx.alignment_statistics()
    M = np.float64(ref["denom"])
    n3 = count.reshape(-1, q, q, q)
    tri = list(itertools.combinations(range(L), 3))
    bound = 2.0 * N * 2.0 ** -41 / meff
    pair = {p: k for k, p in enumerate(itertools.combinations(range(L), 2))}
    worst = 0.0
    for t, (i, j, k) in enumerate(tri):
        worst = max(worst, np.abs(n3[t].sum(axis=(1, 2), dtype=np.uint64).astype(np.float64) / M - xi[i]).max(),
                    np.abs(n3[t].sum(axis=2, dtype=np.uint64).astype(np.float64) / M - xij[pair[i, j]]).max(),
                    np.abs(n3[t].sum(axis=0, dtype=np.uint64).astype(np.float64) / M - xij[pair[j, k]]).max())
    print(name, "implied alignment frequencies: worst difference", worst, "bound", bound)
    assert worst <= bound
    # ... and a set's, bit for bit against dca_sequence_statistics
    _ref, qcount = check_against_brute_force(ctx, X, q, Q, np.ones(300, dtype=np.uint64), name + " set", Ks=(50,))
    yi, yij, _c = ctx.sequence_statistics(Q, compare=False)
    m3 = qcount.reshape(-1, q, q, q)
    for t, (i, j, k) in enumerate(tri):
        assert np.array_equal(bits(m3[t].sum(axis=(1, 2), dtype=np.uint64).astype(np.float64) / 300.0), bits(yi[i]))
        assert np.array_equal(bits(m3[t].sum(axis=(0, 1), dtype=np.uint64).astype(np.float64) / 300.0), bits(yi[k]))
        assert np.array_equal(bits(m3[t].sum(axis=2, dtype=np.uint64).astype(np.float64) / 300.0), bits(yij[pair[i, j]]))
        assert np.array_equal(bits(m3[t].sum(axis=1, dtype=np.uint64).astype(np.float64) / 300.0), bits(yij[pair[i, k]]))
    ctx.close()


def test_identical_columns_tie_in_ascending_element_order():
    rng = np.random.default_rng(21)
    q, L, N = 5, 6, 120
    X = random_alignment(rng, N, L, q)
    X[:, 4] = X[:, 2]                                 # c_{0,2,5} == c_{0,4,5}, c_{1,2,3} == c_{1,3,4} transposed, ...
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.set_weights(np.ones(N))
    el, c3, _f3 = ctx.three_site_scan(400)
    ref = brute_force(X, np.full(N, 2 ** 40, dtype=np.uint64), q)
    rel, rc, _rf = top_elements(ref, L, q, 400)
    assert np.array_equal(el, rel) and np.array_equal(bits(c3), bits(rc))
    lin = ((((el[:, 0].astype(np.int64) * L + el[:, 1]) * L + el[:, 2]) * q + el[:, 3]) * q + el[:, 4]) * q + el[:, 5]
    tied = np.abs(c3[1:]) == np.abs(c3[:-1])
    assert tied.sum() >= 50 and (lin[1:][tied] > lin[:-1][tied]).all()
    # a twin pair by name: (0, 2, 5, a, b, c) and (0, 4, 5, a, b, c) carry the same bits and come in this order
    rows = {tuple(r): n for n, r in enumerate(el.tolist())}
    twins = [(n, rows[(0, 4, 5) + r[3:]]) for r, n in rows.items() if r[:3] == (0, 2, 5) and (0, 4, 5) + r[3:] in rows]
    assert twins and all(bits(c3[a]) == bits(c3[b]) and a < b for a, b in twins)
    ctx.close()


# ---------------------------------------------------------------- 4: split independence
def test_pass_split_and_repetition_leave_every_bit(monkeypatch):
    rng = np.random.default_rng(31)
    q, L = 21, 9
    X = random_alignment(rng, 100, L, q)
    Q = random_alignment(rng, 201, L, q)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    el = all_elements(L, q)[::7]
    base = ctx.three_site_values(el, Q)
    scan = ctx.three_site_scan(300, Q)
    for size in ("7", "64", "200", None):             # DCA_NN_PASS, the pass variable of dca_hamming_nearest, caps the queries per pass
        if size is None:
            monkeypatch.delenv("DCA_NN_PASS")
        else:
            monkeypatch.setenv("DCA_NN_PASS", size)
        out = ctx.three_site_values(el, Q)
        assert np.array_equal(out[0], base[0]) and out[1] == base[1] == 201
        assert np.array_equal(bits(out[2]), bits(base[2])) and np.array_equal(bits(out[3]), bits(base[3]))
        again = ctx.three_site_scan(300, Q)
        assert np.array_equal(again[0], scan[0]) and np.array_equal(bits(again[1]), bits(scan[1])) and np.array_equal(bits(again[2]), bits(scan[2]))
    # repeated rows of `elements` are served, and any subset of the outputs gives the same values
    import ctypes as C
    lib = _lib.lib()
    dup = np.ascontiguousarray(np.concatenate([el[:5], el[:5][::-1]]))
    c = np.zeros(10)
    Qc = np.ascontiguousarray(Q)
    assert lib.dca_three_site_values(ctx._h, Qc.ctypes.data, 201, dup.ctypes.data, 10, None, None, None, c.ctypes.data) == _lib.DCA_OK
    assert np.array_equal(bits(c), bits(np.concatenate([base[3][:5], base[3][:5][::-1]])))
    d = C.c_uint64(0)
    assert lib.dca_three_site_values(ctx._h, Qc.ctypes.data, 201, dup.ctypes.data, 10, None, C.byref(d), None, None) == _lib.DCA_OK and d.value == 201
    ctx.close()


def test_crowded_edge_bin_is_refined_once_then_refused(monkeypatch):
    rng = np.random.default_rng(41)
    q, L, N, K = 5, 9, 257, 300
    X = random_alignment(rng, N, L, q)
    w = 1.0 / rng.integers(1, 9, size=N)
    ref = brute_force(X, quantised_weights(w), q)
    rel, rc, rf = top_elements(ref, L, q, K)
    allc = bits(np.abs(flat(ref, "c3", L)))
    kth = bits(np.abs(rc[K - 1:K]))[0]
    level1 = int((allc >> np.uint64(48) >= kth >> np.uint64(48)).sum())       # candidates of the 15-bit histogram's edge bin and above
    level2 = int((allc >> np.uint64(38) >= kth >> np.uint64(38)).sum())       # ... after the refinement on 10 more mantissa bits
    print("candidates: level 1", level1, "level 2", level2)
    assert K <= level2 < level1
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.set_weights(w)
    for cap in (None, level1, level1 - 1, level2):     # no refinement, none at the cap itself, refinement, refinement that just fits
        if cap is not None:
            monkeypatch.setenv("DCA_THREE_SITE_CAP", str(cap))
        el, c3, f3 = ctx.three_site_scan(K)
        assert np.array_equal(el, rel) and np.array_equal(bits(c3), bits(rc)) and np.array_equal(bits(f3), bits(rf)), cap
    monkeypatch.setenv("DCA_THREE_SITE_CAP", str(level2 - 1))    # still too many after one refinement: refused, nothing allocated
    with pytest.raises(_lib.DcaBackendError) as exc:
        ctx.three_site_scan(K)
    assert exc.value.code == _lib.DCA_ERR_ARG and b"tie with the K-th largest" in _lib.lib().dca_last_error()
    monkeypatch.delenv("DCA_THREE_SITE_CAP")
    # K far into the exact zeros of absent states: the edge is bin 0, everything is appended
    Z = np.ascontiguousarray(X % 2)
    ctx.set_msa(Z, q)
    ctx.set_weights(np.ones(N))
    zref = brute_force(Z, np.full(N, 2 ** 40, dtype=np.uint64), q)
    zel, zc, _zf = top_elements(zref, L, q, 84 * 125 - 100)
    el, c3, _f = ctx.three_site_scan(84 * 125 - 100)
    assert np.array_equal(el, zel) and np.array_equal(bits(c3), bits(zc)) and int((c3 == 0.0).sum()) >= 84 * (125 - 8) - 100
    monkeypatch.setenv("DCA_THREE_SITE_CAP", "9000")             # bin 0 refined on the exponent: the zeros still tie
    with pytest.raises(_lib.DcaBackendError):
        ctx.three_site_scan(84 * 125 - 100)
    ctx.close()


# ---------------------------------------------------------------- 5: classes and the command line
def _unique_records(path):
    recs = fasta_reader.get_alignment_from_fasta_file(path, same_length=False)
    return list(dict.fromkeys(s.upper() for s in recs))


@pytest.mark.parametrize("cls, name, bio", [(PlmDCA, "toy_rna.fa", "rna"), (PlmDCA, "toy_protein.fa", "protein"),
                                            (MeanFieldDCA, "toy_protein.fa", "protein"), (MeanFieldDCA, "toy_rna.fa", "rna"),
                                            (ArDCA, "toy_rna.fa", "rna"), (ArDCA, "toy_protein.fa", "protein")])
def test_own_rows_reproduce_the_alignment(cls, name, bio):
    path = data_file(name)
    rows = _unique_records(path)
    # unit weights, so both sides count the same integers, one scaled by 2^40.  seqid = 1.0 gives them for MeanFieldDCA; the
    # plm weights compare strictly (identity / L > seqid, the reference's rule), so at 1.0 no sequence is similar even to itself
    # and the weights are infinite: there the largest threshold below 1 that no pair of different rows reaches gives unit weights
    inst = cls(path, bio, seqid=1.0 if cls is MeanFieldDCA else 0.99)
    assert np.array_equal(inst._compare_context().weights(), np.ones(len(rows)))
    plain = inst.compare_with_alignment(rows)
    assert set(plain) == TODAYS_KEYS
    res = inst.compare_with_alignment(rows, three_site=500)
    assert set(res) == TODAYS_KEYS | {"pearson_cijk", "slope_cijk", "max_abs_diff_cijk", "three_site_terms"}
    assert all(np.array_equal(plain[k], res[k]) for k in plain)
    print(cls.__name__, name, res["pearson_cijk"], res["slope_cijk"], res["max_abs_diff_cijk"])
    assert abs(res["pearson_cijk"] - 1.0) <= 1e-12 and abs(res["slope_cijk"] - 1.0) <= 1e-12
    assert res["max_abs_diff_cijk"] <= 4e-15 and res["three_site_terms"] == 500
    nogap = inst.compare_with_alignment(rows, three_site=500, three_site_include_gaps=False)
    assert abs(nogap["pearson_cijk"] - 1.0) <= 1e-12 and nogap["three_site_terms"] == 500


def test_meanfield_class_against_the_brute_force():
    path = data_file("toy_protein.fa")
    inst = MeanFieldDCA(path, "protein")
    X = fasta_reader.get_alignment_int_array(path, biomolecule="PROTEIN", zero_based=True)
    ctx = inst._compare_context()
    assert np.array_equal(ctx.hamming_nearest(np.ascontiguousarray(X, dtype=np.uint8))[0], np.zeros(X.shape[0], dtype=np.int32))
    ref = brute_force(X, quantised_weights(ctx.weights()), 21)
    for gaps, skip in ((True, -1), (False, 20)):
        top = inst.compute_top_three_site_correlations(200, include_gaps=gaps)
        rel, rc, rf = top_elements(ref, 8, 21, 200, skip)
        assert top["elements"].dtype == np.int32 and np.array_equal(top["elements"], rel)
        assert np.array_equal(bits(top["c3"]), bits(rc)) and np.array_equal(bits(top["f3"]), bits(rf))
        assert gaps or not (top["elements"][:, 3:] == 20).any()
        f3, c3 = inst.compute_three_site_correlations(top["elements"])
        assert np.array_equal(bits(f3), bits(rf)) and np.abs(c3 - rc).max() <= 4e-15
    rows = _unique_records(path)[:20]
    Q = _lib.encode_sequences(rows, _lib.DCA_BIOMOLECULE_PROTEIN, 8, 1)
    qref = brute_force(Q, np.ones(20, dtype=np.uint64), 21)
    top = inst.compute_top_three_site_correlations(30, sequences=rows)
    rel, rc, _rf = top_elements(qref, 8, 21, 30)
    assert np.array_equal(top["elements"], rel) and np.array_equal(bits(top["c3"]), bits(rc))


def test_ardca_and_plmdca_agree_in_file_order():
    path = data_file("toy_rna.fa")
    rows = _unique_records(path)[5:30]
    ar, plm = ArDCA(path, "rna"), PlmDCA(path, "rna")
    assert not np.array_equal(ar.site_order, np.arange(10))            # the model order permutes this alignment's sites
    total = 120 * 125
    for seqs in (None, rows):
        a = ar.compute_top_three_site_correlations(total, sequences=seqs)
        p = plm.compute_top_three_site_correlations(total, sequences=seqs)
        assert a["elements"].shape == p["elements"].shape == (total, 6)
        assert (a["elements"][:, 0] < a["elements"][:, 1]).all() and (a["elements"][:, 1] < a["elements"][:, 2]).all()
        oa, op = np.lexsort(a["elements"].T[::-1]), np.lexsort(p["elements"].T[::-1])
        assert np.array_equal(a["elements"][oa], p["elements"][op])                 # ties may order differently: sorted first
        assert np.abs(a["c3"][oa] - p["c3"][op]).max() <= 4e-15 and np.array_equal(bits(a["f3"][oa]), bits(p["f3"][op]))
        # the strongest elements, asked for by name in file order, from both classes
        el = p["elements"][:300]
        fa, ca = ar.compute_three_site_correlations(el, sequences=seqs)
        fp, cp = plm.compute_three_site_correlations(el, sequences=seqs)
        assert np.array_equal(bits(fa), bits(fp)) and np.array_equal(bits(fp), bits(p["f3"][:300]))
        assert np.abs(ca - cp).max() <= 4e-15 and np.abs(cp - p["c3"][:300]).max() <= 4e-15
    ra, rp = ar.compare_with_alignment(rows, three_site=400), plm.compare_with_alignment(rows, three_site=400)
    assert ra["three_site_terms"] == rp["three_site_terms"] == 400
    assert 0.0 < rp["pearson_cijk"] <= 1.0 and np.isfinite(rp["slope_cijk"]) and rp["max_abs_diff_cijk"] > 0.0


def test_command_line_writes_the_new_lines_only_when_asked(tmp_path):
    path = data_file("toy_rna.fa")
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as fh:
        fh.writelines(">q{}\n{}\n".format(k, s) for k, s in enumerate(_unique_records(path)[:15]))
    plain = plmdca_main.run_plm_dca(["compare_sequences", "rna", path, "--query_file", qfile, "--output_dir", str(tmp_path / "a")])
    with3 = plmdca_main.run_plm_dca(["compare_sequences", "rna", path, "--query_file", qfile, "--output_dir", str(tmp_path / "b"),
                                     "--three_site", "250", "--three_site_no_gaps"])
    a, b = open(plain).read().splitlines(), open(with3).read().splitlines()
    new = [ln for ln in b if ln not in a]
    assert [ln.split(":")[0] for ln in new] == ["#\tmax_abs_diff_cijk", "#\tpearson_cijk", "#\tslope_cijk", "#\tthree_site_terms"]
    assert new[3] == "#\tthree_site_terms: 250" and [ln for ln in b if ln in a] == a
    assert os.path.basename(plain) == os.path.basename(with3)


# ---------------------------------------------------------------- 6: errors
def test_argument_and_state_errors():
    import ctypes as C
    lib = _lib.lib()
    found = C.c_int(0)
    out, c = np.zeros((4, 6), dtype=np.int32), np.zeros(4)
    el = np.array([[0, 1, 2, 0, 0, 0]], dtype=np.int32)

    def values(ctx, e, Q=None, nq=0):
        e = np.ascontiguousarray(e, dtype=np.int32)
        return lib.dca_three_site_values(ctx._h, None if Q is None else Q.ctypes.data, nq, e.ctypes.data, e.shape[0], None, None, None, c.ctypes.data)

    def scan(ctx, K=4, Q=None, nq=0, skip=-1):
        return lib.dca_three_site_scan(ctx._h, None if Q is None else Q.ctypes.data, nq, K, skip, out.ctypes.data, c.ctypes.data, None, C.byref(found))

    ctx = _lib.Context(0, _lib.DCA_F64)
    assert values(ctx, el) == _lib.DCA_ERR_STATE and scan(ctx) == _lib.DCA_ERR_STATE            # no alignment
    assert b"dca_set_msa first" in lib.dca_last_error()
    two = np.zeros((4, 2), dtype=np.uint8)
    ctx.set_msa(two, 5)
    ctx.set_weights(np.ones(4))
    assert values(ctx, el) == _lib.DCA_ERR_ARG and scan(ctx) == _lib.DCA_ERR_ARG                # L = 2
    assert b"three sites" in lib.dca_last_error()
    X = np.random.default_rng(0).integers(0, 5, size=(6, 4), dtype=np.uint8)
    ctx.set_msa(X, 5)
    assert values(ctx, el) == _lib.DCA_ERR_STATE and scan(ctx) == _lib.DCA_ERR_STATE            # Q NULL, no weights yet
    assert b"dca_compute_weights or dca_set_weights first" in lib.dca_last_error()
    assert values(ctx, el, X, 6) == _lib.DCA_OK and scan(ctx, 4, X, 6) == _lib.DCA_OK and found.value == 4     # a set needs none
    ctx.compute_weights(0.8, _lib.DCA_F64)
    assert values(ctx, el) == _lib.DCA_OK
    for bad in ([[0, 2, 1, 0, 0, 0]], [[1, 1, 2, 0, 0, 0]], [[0, 1, 4, 0, 0, 0]], [[-1, 1, 2, 0, 0, 0]], [[0, 1, 2, 0, 0, 0], [2, 1, 3, 0, 0, 0]]):
        assert values(ctx, bad) == _lib.DCA_ERR_ARG and b"0 <= i < j < k < 4" in lib.dca_last_error(), bad
    for bad in ([[0, 1, 2, 5, 0, 0]], [[0, 1, 2, 0, 0, -1]], [[0, 1, 2, 0, 31, 0]]):
        assert values(ctx, bad) == _lib.DCA_ERR_ARG and b"states are 0 .. 4" in lib.dca_last_error(), bad
    badQ = X.copy()
    badQ[3, 2] = 5
    assert values(ctx, el, badQ, 6) == _lib.DCA_ERR_ARG and b"code 5 >= q" in lib.dca_last_error()
    assert scan(ctx, 4, badQ, 6) == _lib.DCA_ERR_ARG
    assert scan(ctx, 0) == _lib.DCA_ERR_ARG and scan(ctx, -2) == _lib.DCA_ERR_ARG               # K < 1
    assert scan(ctx, 4, X, 0) == _lib.DCA_ERR_ARG and values(ctx, el, X, 0) == _lib.DCA_ERR_ARG  # nq < 1 with Q
    assert scan(ctx, 4, skip=5) == _lib.DCA_ERR_ARG and scan(ctx, 4, skip=-2) == _lib.DCA_ERR_ARG
    assert lib.dca_three_site_values(ctx._h, None, 0, el.ctypes.data, 0, None, None, None, c.ctypes.data) == _lib.DCA_ERR_ARG   # T < 1
    assert lib.dca_three_site_values(ctx._h, None, 0, el.ctypes.data, 1, None, None, None, None) == _lib.DCA_ERR_ARG            # no output
    assert lib.dca_three_site_scan(ctx._h, None, 0, 4, -1, None, c.ctypes.data, None, C.byref(found)) == _lib.DCA_ERR_ARG
    assert scan(ctx) == _lib.DCA_OK and found.value == 4                                          # the context still serves
    ctx.close()
