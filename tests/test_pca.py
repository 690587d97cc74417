"""Principal components of the reweighted alignment and projections of sequence sets on the GPU (dca_pca_fit, dca_pca_project,
the class methods and the command lines) against tests/pca_reference.py: the one-hot covariance as the
contract defines it with numpy.linalg.eigh, and the projection in the contract's order.

Bounds.  eps = 64 L q 2^-53 lambda_1 stands for the rounding of the reference; res_m is the residual the fit reports.
  eigenvalues   |lambda_m - lambda_ref,m| <= res_m + eps (an eigenvalue of a symmetric matrix lies within the residual norm)
  vectors       ||v_m - v_ref,m|| <= 2 (res_m + eps) / gap_m wherever gap_m >= 0.01 lambda_1 (Davis-Kahan)
  projections   bit for bit the ordered sum, alone, in any batch, under any pass split
  moments       <= 2^-53 (2 L N + 64 L q lambda_1) + res
The synthetic alignments carry planted modes (pca_reference.planted_alignment); their seeds were chosen so that every
compared component has a gap of at least 0.03 lambda_1 under both weightings, and the test asserts the 0.01 on the reference.
One variant cannot meet it and is left out of the vector check: at L = 1 the weights of dca_compute_weights(0.8) are one over
the number of identical rows, every state present then has the total weight 1, the frequencies are uniform and all non-zero
eigenvalues of C coincide.  Its eigenvalues, residuals, projections and moments are checked like everybody's."""
import os

import numpy as np
import pytest

from conftest import ROOT, data_file
import pca_reference as ref
from pydca_amd import _lib, ardca_main, mfdca_main, plmdca_main
from pydca_amd.ardca.ardca import ArDCA, ArDCAException
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

pytestmark = pytest.mark.gpu

TOL = 1e-10
SLAB = _lib.PCA_SLAB
# (q, L, N, k): generator seed
SHAPES = {(21, 1, 63, 2): 0, (21, 2, 1, 1): 0, (5, 9, 6, 4): 0, (5, 3, 63, 7): 2, (21, 3, 63, 2): 0, (21, 7, 257, 3): 0,
          (5, 17, 513, 4): 0, (5, 33, 2049, 2): 0, (32, 5, 63, 2): 0, (21, 40, 1000, 4): 0, (21, 40, 300, 64): 0,
          (21, 7, SLAB - 1, 3): 0, (21, 7, SLAB, 3): 0, (21, 7, SLAB + 1, 3): 0}
TODAYS_KEYS = {"num_sequences", "nearest_distance", "nearest_distance_mean", "nearest_distance_median", "nearest_distance_min",
               "fraction_identical", "alignment_self_distance_mean", "alignment_self_distance_median", "alignment_self_distance_min"} | {
                   "{}_{}".format(n, w) for n in ("pearson", "slope", "max_abs_diff") for w in ("fi", "fij", "cij")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check_fit(fit, X, w, q, k, what, vectors=True, need_gaps=True, reference=None):
    """checks 1, 2, 3 and the trace of 5 of one fit against the reference of (X, w); -> (lam_ref, V_ref, C, f, eps)"""
    N, L = X.shape
    rows = L * q
    lam_ref, V_ref, Cm, f = reference if reference is not None else ref.eigh(X, w, q)
    lam1 = lam_ref[0]
    eps = 64 * rows * 2.0 ** -53 * lam1
    lam, V, res = fit["eigenvalues"], fit["components"].reshape(k, rows), fit["residuals"]
    assert fit["converged"], what
    null = np.array([not V[m].any() for m in range(k)])
    # ---- 1: the contract
    print(what, "iterations", fit["iterations"], "max res / lambda_1", (res.max() / lam1) if lam1 > 0 else 0.0)
    assert np.all(res <= TOL * lam[0]), what
    assert np.all(np.diff(lam) <= 0) and np.all(lam >= 0), what
    worst_again = -np.inf
    for m in range(k):
        if null[m]:
            assert lam[m] == 0.0 and fit["offsets"][m] == 0.0, (what, m)
        else:
            assert lam[m] > TOL * lam[0], (what, m)
            at = int(np.argmax(np.abs(V[m])))
            assert V[m, at] > 0.0, (what, m)                                  # the sign rule, ties to the smallest index
        assert not (lam_ref[m] > 1e-8 * lam1 and null[m]) and not (lam_ref[m] < 1e-12 * lam1 and not null[m]), (what, m)
        again = np.linalg.norm(Cm @ V[m] - lam[m] * V[m])
        worst_again = max(worst_again, again - res[m])
        assert again <= res[m] + eps, (what, m, again, res[m], eps)
    print(what, "max (recomputed residual - reported)", worst_again, "eps", eps)
    live = V[~null]
    if live.size:
        orth = np.abs(live @ live.T - np.eye(live.shape[0])).max()
        print(what, "max |V V^T - I|", orth, "bound", 8 * rows * 2.0 ** -53)
        assert orth <= 8 * rows * 2.0 ** -53, what
    assert np.abs(fit["offsets"] - V @ f).max() <= 64 * rows * 2.0 ** -53, what
    # ---- 2: eigenvalues
    err = np.abs(lam - lam_ref[:k])
    print(what, "max |lambda - ref| / lambda_1", (err.max() / lam1) if lam1 > 0 else 0.0)
    assert np.all(err <= res + eps), (what, err, res, eps)
    # ---- 3: vectors
    if vectors:
        gap = ref.gaps(lam_ref)[:k]
        worst = 0.0
        for m in range(k):
            if null[m]:
                continue
            if need_gaps:
                assert gap[m] >= 0.01 * lam1, (what, m, gap[m] / lam1)           # on the reference alone: the seed's promise
            if gap[m] >= 0.01 * lam1:
                d = np.linalg.norm(V[m] - V_ref[m])
                worst = max(worst, d / (2 * (res[m] + eps) / gap[m]))
                assert d <= 2 * (res[m] + eps) / gap[m], (what, m, d, res[m], eps, gap[m])
        print(what, "max vector error / Davis-Kahan bound", worst, "min compared gap / lambda_1",
              min([gap[m] / lam1 for m in range(k) if not null[m] and gap[m] >= 0.01 * lam1], default=float("nan")))
    # ---- 5: the trace
    assert lam.sum() <= fit["total_variance"] * (1 + 1e-12) + eps, what
    assert abs(fit["total_variance"] - np.trace(Cm)) <= eps, what
    return lam_ref, V_ref, Cm, f, eps


def check_moments(fit, P, w, X, q, k, eps, what):
    """check 5: the alignment's projections have the weighted mean 0 and the weighted covariance diag(lambda)"""
    N, L = X.shape
    lam, res = fit["eigenvalues"], fit["residuals"]
    lam1 = lam[0]
    base = 2.0 ** -53 * (2 * L * N + 64 * L * q * lam1)
    meff = w.sum()
    mean = np.abs((w[:, None] * P).sum(axis=0) / meff)
    cov = np.abs((P * w[:, None]).T @ P / meff - np.diag(lam))
    bound = base + np.minimum(res[:, None], res[None, :])
    print(what, "max weighted |mean|", mean.max(), "max |cov - diag(lambda)|", cov.max(), "bound", base)
    assert np.all(mean <= base + res), what
    assert np.all(cov <= bound), what


def check_projections(ctx, fit, X, q, monkeypatch, what):
    """check 4: the ordered sum, bit for bit, for the alignment and a 700-row set; alone, in batches, under pass splits"""
    comps, offs = fit["components"], fit["offsets"]
    L = X.shape[1]
    P = ctx.pca_project(comps, offs)
    assert same_bits(P, ref.project(X, comps, offs)), what
    Q = np.random.default_rng(5).integers(0, q, size=(700, L), dtype=np.uint8)
    Q[:X.shape[0]][:50] = X[:50]
    want = ref.project(Q, comps, offs)
    assert same_bits(ctx.pca_project(comps, offs, Q), want), what
    for k in range(0, 70, 3):
        assert same_bits(ctx.pca_project(comps, offs, Q[k:k + 1]), want[k:k + 1]), (what, "alone", k)
    for batch in (7, 64):
        for first in range(0, 2 * batch + 3, batch):
            assert same_bits(ctx.pca_project(comps, offs, Q[first:first + batch]), want[first:first + batch]), (what, batch, first)
    for split in (7, 200):
        monkeypatch.setenv("DCA_NN_PASS", str(split))
        assert same_bits(ctx.pca_project(comps, offs, Q), want), (what, "DCA_NN_PASS", split)
    monkeypatch.delenv("DCA_NN_PASS")
    return P


@pytest.mark.parametrize("q, L, N, k", list(SHAPES), ids=lambda v: str(v))
def test_synthetic_alignments(q, L, N, k, monkeypatch):
    seed = SHAPES[(q, L, N, k)]
    X = ref.planted_alignment(q, L, N, k, seed)
    big = k == 64                                                 # k at its cap: eigenvalues and the contract, no vectors
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    what = ("weights(0.8)", q, L, N, k)
    fit = ctx.pca_fit(k, TOL, 1000, 0)
    _lr, _Vr, _C, _f, eps = check_fit(fit, X, w, q, k, what, vectors=not big, need_gaps=L > 1)
    P = check_projections(ctx, fit, X, q, monkeypatch, what)
    check_moments(fit, P, w, X, q, k, eps, what)
    assert same_bits(ctx.weights(), w)                            # 7: nothing else moved
    if N == 1:
        assert fit["iterations"] == 0 and not fit["components"].any() and not P.any()
    if not big:
        # ---- 6: the same arguments give the same bits; another seed the same eigenvalues within the residuals
        twin = ctx.pca_fit(k, TOL, 1000, 0)
        for key in ("eigenvalues", "components", "offsets", "residuals"):
            assert same_bits(fit[key], twin[key]), (what, key)
        assert twin["iterations"] == fit["iterations"] and same_bits([twin["total_variance"]], [fit["total_variance"]])
        other = ctx.pca_fit(k, TOL, 1000, 12345)
        assert other["converged"], what
        assert np.all(np.abs(other["eigenvalues"] - fit["eigenvalues"]) <= other["residuals"] + fit["residuals"] + 2 * eps), what
        # ---- the second weighting: random values in (0, 1]
        w2 = 1.0 - np.random.default_rng(seed + 1000).random(N)
        ctx.set_weights(w2)
        what2 = ("random weights", q, L, N, k)
        fit2 = ctx.pca_fit(k, TOL, 1000, 0)
        _lr, _Vr, _C, _f, eps2 = check_fit(fit2, X, w2, q, k, what2)
        P2 = ctx.pca_project(fit2["components"], fit2["offsets"])
        assert same_bits(P2, ref.project(X, fit2["components"], fit2["offsets"])), what2
        check_moments(fit2, P2, w2, X, q, k, eps2, what2)
        assert same_bits(ctx.weights(), w2)
    ctx.close()


def test_out_of_iterations_is_reported_not_raised():
    X = ref.planted_alignment(21, 7, 257, 3, 0)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, 21)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    fit = ctx.pca_fit(3, TOL, 2, 0)
    assert not fit["converged"] and fit["iterations"] == 2 and fit["residuals"].max() > TOL * fit["eigenvalues"][0]
    lam_ref, _V, Cm, _f = ref.eigh(X, w, 21)
    eps = 64 * 147 * 2.0 ** -53 * lam_ref[0]
    V = fit["components"].reshape(3, 147)
    for m in range(3):                   # the residuals it returns are those of what it returns; SOME eigenvalue lies that near
        again = np.linalg.norm(Cm @ V[m] - fit["eigenvalues"][m] * V[m])
        assert again <= fit["residuals"][m] + eps and np.abs(fit["eigenvalues"][m] - lam_ref).min() <= fit["residuals"][m] + eps
    ctx.close()


def test_fitted_model_is_untouched():
    G = np.load(os.path.join(ROOT, "tests", "golden", "plm_toy_rna.npz"))
    X, q = G["X"], int(G["q"])
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    fx = ctx.plm_gradient()
    x, g = ctx.plm_get_x(np.float32), ctx.plm_get_g(np.float32)
    fit = ctx.pca_fit(2, TOL, 1000, 0)
    assert fit["converged"]
    ctx.pca_project(fit["components"], fit["offsets"], X[:7])
    assert np.array_equal(ctx.plm_get_x(np.float32), x) and np.array_equal(ctx.plm_get_g(np.float32), g)
    assert same_bits(ctx.weights(), w) and ctx.plm_gradient() == fx
    ctx.close()


# ---------------------------------------------------------------- the real alignment
def test_pf02826_through_the_class(monkeypatch):
    path = data_file("PF02826.faa")
    inst = PlmDCA(path, "protein")
    ctx = inst._compare_context()
    w = ctx.weights()
    recs = fasta_reader.get_alignment_from_fasta_file(path, same_length=False)
    rows = list(dict.fromkeys(s.upper() for s in recs))
    X = _lib.encode_sequences(rows, _lib.DCA_BIOMOLECULE_PROTEIN, inst.sequences_len, 0)
    assert X.shape[0] == w.size
    k, q = 10, 21
    out = inst.compute_principal_components(num_components=k)
    assert set(out) == {"eigenvalues", "components", "offsets", "explained_variance_ratio", "total_variance", "residuals", "iterations"}
    assert out["components"].shape == (k, X.shape[1], q)
    fit = dict(out, converged=True)
    _lr, _Vr, _C, _f, eps = check_fit(fit, X, w, q, k, ("PF02826", k), need_gaps=False)
    assert np.allclose(out["explained_variance_ratio"], out["eigenvalues"] / out["total_variance"], rtol=1e-15, atol=0)
    P = inst.project_sequences(None, num_components=k)
    assert same_bits(P, ref.project(X, out["components"], out["offsets"]))
    check_moments(fit, P, w, X, q, k, eps, "PF02826")
    assert same_bits(inst.project_sequences(rows[:9], num_components=k), P[:9])          # the same rows as a query set
    assert inst.compute_principal_components(num_components=k)["iterations"] == out["iterations"]


# ---------------------------------------------------------------- 8: classes and command lines
def _unique_records(path):
    recs = fasta_reader.get_alignment_from_fasta_file(path, same_length=False)
    return list(dict.fromkeys(s.upper() for s in recs))


@pytest.mark.parametrize("name, bio, q", [("toy_rna.fa", "rna", 5), ("toy_protein.fa", "protein", 21)])
def test_plmdca_and_ardca_agree_in_file_order(name, bio, q):
    path = data_file(name)
    rows = _unique_records(path)
    plm, ar = PlmDCA(path, bio), ArDCA(path, bio)
    L = plm.sequences_len
    X = _lib.encode_sequences(rows, _lib.DCA_BIOMOLECULE_RNA if bio == "rna" else _lib.DCA_BIOMOLECULE_PROTEIN, L, 0)
    w = plm._compare_context().weights()
    assert np.array_equal(w, ar._compare_context().weights())                        # the same de-duplicated rows
    k = 3
    p, a = plm.compute_principal_components(k), ar.compute_principal_components(k)
    assert p["components"].shape == a["components"].shape == (k, L, q)
    reference = ref.eigh(X, w, q)
    lam_ref, _V, _C, _f, eps = check_fit(dict(p, converged=True), X, w, q, k, ("PlmDCA", name), need_gaps=False, reference=reference)
    check_fit(dict(a, converged=True), X, w, q, k, ("ArDCA", name), need_gaps=False, reference=reference)   # in FILE order
    assert np.all(np.abs(p["eigenvalues"] - a["eigenvalues"]) <= p["residuals"] + a["residuals"] + 2 * eps)
    gap = ref.gaps(lam_ref)[:k]
    for m in range(k):
        if gap[m] >= 0.01 * lam_ref[0]:
            d = np.linalg.norm(p["components"][m] - a["components"][m])
            assert d <= 2 * (p["residuals"][m] + a["residuals"][m] + 2 * eps) / gap[m], (name, m, d)
    # projections: each class projects with its own components.  PlmDCA's context holds the sites in file order, so the
    # reference's ordered sum is met bit for bit; ArDCA's chain runs over the sites in MODEL order, the same L terms of magnitude
    # <= 1 in another order: two chains of L - 1 roundings each on partial sums <= L
    pp, pa = plm.project_sequences(rows[:40], k), ar.project_sequences(rows[:40], k)
    assert same_bits(pp, ref.project(X[:40], p["components"], p["offsets"]))
    assert np.abs(pa - ref.project(X[:40], a["components"], a["offsets"])).max() <= 2 * L * L * 2.0 ** -53
    assert same_bits(pa, ar.project_sequences(None, k)[:40]) and same_bits(pa[3:4], ar.project_sequences(rows[3:4], k))
    if bio == "rna":
        assert not np.array_equal(ar.site_order, np.arange(L))                      # the model order permutes this alignment's sites


@pytest.mark.parametrize("name, bio, q", [("toy_rna.fa", "rna", 5), ("toy_protein.fa", "protein", 21)])
def test_meanfield_class_against_its_own_rows(name, bio, q):
    path = data_file(name)
    inst = MeanFieldDCA(path, bio)
    X = np.ascontiguousarray(fasta_reader.get_alignment_int_array(path, biomolecule=bio.upper(), zero_based=True), dtype=np.uint8)
    ctx = inst._compare_context()
    w = ctx.weights()
    assert X.shape[0] == w.size
    k = 2
    out = inst.compute_principal_components(k)
    _lr, _Vr, _C, _f, eps = check_fit(dict(out, converged=True), X, w, q, k, ("MeanFieldDCA", name), need_gaps=False)
    P = inst.project_sequences(None, k)
    assert same_bits(P, ref.project(X, out["components"], out["offsets"]))
    check_moments(dict(out, converged=True), P, w, X, q, k, eps, ("MeanFieldDCA", name))


@pytest.mark.parametrize("cls", [PlmDCA, MeanFieldDCA, ArDCA])
def test_compare_with_alignment_gains_three_keys(cls):
    path = data_file("toy_rna.fa")
    rows = _unique_records(path)
    # unit weights (see tests/test_three_site.py: the plm weights compare strictly, so 0.99 gives them where 1.0 cannot)
    inst = cls(path, "rna", seqid=1.0 if cls is MeanFieldDCA else 0.99)
    w = inst._compare_context().weights()
    assert np.array_equal(w, np.ones(len(rows)))
    plain = inst.compare_with_alignment(rows)
    assert set(plain) == TODAYS_KEYS
    assert set(inst.compare_with_alignment(rows, pca=0)) == TODAYS_KEYS
    res = inst.compare_with_alignment(rows, pca=2)
    assert set(res) == TODAYS_KEYS | {"pca_eigenvalues", "pca_set_mean", "pca_set_variance"}
    assert all(np.array_equal(plain[key], res[key]) for key in plain)
    fit = inst.compute_principal_components(2)
    assert same_bits(res["pca_eigenvalues"], fit["eigenvalues"])
    N, L, q = len(rows), 10, 5
    lam1 = fit["eigenvalues"][0]
    bound = 2.0 ** -53 * (2 * L * N + 64 * L * q * lam1) + fit["residuals"]
    print(cls.__name__, "set mean", res["pca_set_mean"], "variance - lambda", res["pca_set_variance"] - fit["eigenvalues"], "bound", bound)
    assert res["pca_set_mean"].shape == res["pca_set_variance"].shape == (2,)
    assert np.all(np.abs(res["pca_set_mean"]) <= bound)
    assert np.all(np.abs(res["pca_set_variance"] - fit["eigenvalues"]) <= bound + bound ** 2)


@pytest.mark.parametrize("main, prefix", [("plm", "PLMDCA"), ("mf", "MFDCA"), ("ar", "ARDCA")])
def test_command_line_writes_the_four_files(tmp_path, main, prefix):
    run = {"plm": plmdca_main.run_plm_dca, "mf": mfdca_main.run_meanfield_dca, "ar": ardca_main.run_ardca}[main]
    path = data_file("toy_protein.fa")
    rows = _unique_records(path)
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as fh:
        fh.writelines(">q{}\n{}\n".format(n, s) for n, s in enumerate(rows[:15]))
    out = str(tmp_path / "out")
    files = run(["compute_pca", "protein", path, "--num_components", "3", "--query_file", qfile, "--seed", "1", "--output_dir", out])
    assert [os.path.basename(f) for f in files] == [prefix + "_pca_toy_protein.txt", prefix + "_pca_components_toy_protein.npy",
                                                    prefix + "_pca_projections_toy_protein.txt",
                                                    prefix + "_pca_query_projections_toy_protein.txt"]
    table = lambda f: [ln.split() for ln in open(f).read().splitlines() if not ln.startswith("#")]
    summary = table(files[0])
    assert [r[0] for r in summary] == ["1", "2", "3"] and all(len(r) == 4 for r in summary)
    lam = np.array([float(r[1]) for r in summary])
    assert np.all(np.diff(lam) <= 0) and lam[0] > 0 and all(0 <= float(r[2]) <= 1 for r in summary)
    assert any(ln.startswith("#\tIterations: ") for ln in open(files[0]))
    comps = np.load(files[1])
    L = comps.shape[1]
    assert comps.shape == (3, L, 21) and comps.dtype == np.float64
    assert np.abs(comps.reshape(3, -1) @ comps.reshape(3, -1).T - np.eye(3)).max() <= 8 * L * 21 * 2.0 ** -53
    proj = table(files[2])
    n_rows = len(proj)
    assert n_rows >= len(rows) and all(len(r) == 2 + 3 for r in proj) and [int(r[0]) for r in proj] == list(range(n_rows))
    wts = np.array([float(r[1]) for r in proj])
    P = np.array([[float(v) for v in r[2:]] for r in proj])
    assert np.all(wts > 0) and np.all(wts <= 1)
    assert np.abs((wts[:, None] * P).sum(axis=0) / wts.sum()).max() <= 1e-12       # %.17g reads back: weighted mean 0
    assert np.allclose((wts[:, None] * P * P).sum(axis=0) / wts.sum(), lam, rtol=0, atol=1e-9 * lam[0])
    qp = table(files[3])
    assert len(qp) == 15 and all(len(r) == 1 + 3 for r in qp) and [int(r[0]) for r in qp] == list(range(1, 16))
    three = run(["compute_pca", "protein", path, "--output_dir", str(tmp_path / "plain")])      # the defaults: 2 components, no queries
    assert len(three) == 3 and np.load(three[1]).shape == (2, L, 21)
    # compare_sequences --pca K: three header lines per component, nothing else new
    plain = run(["compare_sequences", "protein", path, "--query_file", qfile, "--output_dir", str(tmp_path / "c0")])
    with_pca = run(["compare_sequences", "protein", path, "--query_file", qfile, "--output_dir", str(tmp_path / "c2"), "--pca", "2"])
    a, b = open(plain).read().splitlines(), open(with_pca).read().splitlines()
    assert sorted(ln.split(":")[0] for ln in b if ln not in a) == sorted(
        "#\t{}_{}".format(key, m) for key in ("pca_eigenvalues", "pca_set_mean", "pca_set_variance") for m in (1, 2))
    assert [ln for ln in b if ln in a] == a


def test_several_devices_are_refused():
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", devices=[0, 1])
    for call in (inst.compute_principal_components, inst.project_sequences, lambda: inst.compare_with_alignment(["ACGUACGUAC"], pca=2)):
        with pytest.raises(PlmDCAException, match="one GPU"):
            call()


def test_a_fit_out_of_iterations_raises_in_the_class():
    for cls, exc in ((PlmDCA, PlmDCAException), (MeanFieldDCA, MeanFieldDCAException), (ArDCA, ArDCAException)):
        inst = cls(data_file("toy_protein.fa"), "protein")
        with pytest.raises(exc, match="did not converge in 1 iterations: component"):
            inst.compute_principal_components(2, max_iterations=1)


# ---------------------------------------------------------------- 9: errors
def test_argument_and_state_errors():
    import ctypes as C
    lib = _lib.lib()
    lam, off, res = np.zeros(64), np.zeros(64), np.zeros(64)
    comp, proj = np.zeros(64 * 20), np.zeros(6 * 64)
    total, it, conv = C.c_double(0), C.c_int(0), C.c_int(0)

    def fit(ctx, k=2, tol=1e-10, iters=50, lam_=lam, comp_=comp, off_=off, conv_=conv):
        return lib.dca_pca_fit(ctx._h, k, tol, iters, 0, None if lam_ is None else lam_.ctypes.data,
                               None if comp_ is None else comp_.ctypes.data, None if off_ is None else off_.ctypes.data, res.ctypes.data,
                               C.byref(total), C.byref(it), None if conv_ is None else C.byref(conv_))

    def project(ctx, Q=None, nq=0, k=2, comp_=comp, off_=off, out_=proj):
        return lib.dca_pca_project(ctx._h, None if Q is None else Q.ctypes.data, nq, k, None if comp_ is None else comp_.ctypes.data,
                                   None if off_ is None else off_.ctypes.data, None if out_ is None else out_.ctypes.data)

    ctx = _lib.Context(0, _lib.DCA_F64)
    assert fit(ctx) == _lib.DCA_ERR_STATE and project(ctx) == _lib.DCA_ERR_STATE              # no alignment
    assert b"dca_set_msa first" in lib.dca_last_error()
    X = np.random.default_rng(0).integers(0, 5, size=(6, 4), dtype=np.uint8)
    ctx.set_msa(X, 5)
    assert fit(ctx) == _lib.DCA_ERR_STATE                                                      # no weights
    assert b"dca_compute_weights or dca_set_weights first" in lib.dca_last_error()
    assert project(ctx) == _lib.DCA_OK and project(ctx, X, 6) == _lib.DCA_OK                   # projecting needs none
    ctx.compute_weights(0.8, _lib.DCA_F64)
    assert fit(ctx) == _lib.DCA_OK and conv.value == 1
    for k in (0, -1, 21, 65):                                                                  # L q = 20
        assert fit(ctx, k=k) == _lib.DCA_ERR_ARG, k
    assert fit(ctx, k=20) == _lib.DCA_OK                                                       # k = L q itself is served
    for tol in (0.0, -1e-3, float("nan")):
        assert fit(ctx, tol=tol) == _lib.DCA_ERR_ARG, tol
    assert fit(ctx, iters=0) == _lib.DCA_ERR_ARG and fit(ctx, iters=-3) == _lib.DCA_ERR_ARG
    assert fit(ctx, lam_=None) == _lib.DCA_ERR_ARG and fit(ctx, comp_=None) == _lib.DCA_ERR_ARG
    assert fit(ctx, off_=None) == _lib.DCA_ERR_ARG and fit(ctx, conv_=None) == _lib.DCA_ERR_ARG
    assert lib.dca_pca_fit(ctx._h, 2, 1e-10, 50, 0, lam.ctypes.data, comp.ctypes.data, off.ctypes.data, None, None, None,
                           C.byref(conv)) == _lib.DCA_OK                                       # the optional outputs
    assert project(ctx, k=0) == _lib.DCA_ERR_ARG
    assert project(ctx, comp_=None) == _lib.DCA_ERR_ARG and project(ctx, off_=None) == _lib.DCA_ERR_ARG
    assert project(ctx, out_=None) == _lib.DCA_ERR_ARG
    assert project(ctx, X, 0) == _lib.DCA_ERR_ARG and project(ctx, X, -1) == _lib.DCA_ERR_ARG   # nq < 1 with Q
    badQ = X.copy()
    badQ[3, 2] = 5
    assert project(ctx, badQ, 6) == _lib.DCA_ERR_ARG and b"code 5 >= q" in lib.dca_last_error()
    assert fit(ctx) == _lib.DCA_OK and project(ctx, X, 6) == _lib.DCA_OK                       # the context still serves
    ctx.close()
