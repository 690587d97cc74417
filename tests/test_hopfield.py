"""The Hopfield-Potts entries on the device (dca_mf_hopfield_fit, dca_mf_hopfield_couplings, dca_mf_model_kind,
dca_hopfield_project, dca_dense_apply) against tests/hopfield_reference.py.  Bounds: eps is the measured
rounding of the reference (two float64 formulations, margin 8; hopfield_reference.epsilon), r_mu the residual the fit reports;
the derived ones are stated where they are used and in hopfield_cases.py.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest

from conftest import assert_scores_within, data_file, golden
from oracle import mf as omf
import hopfield_cases as hc
import hopfield_reference as href
from pydca_amd import _lib, hopfield_main
from pydca_amd.hopfield_dca.hopfield_dca import HopfieldPottsDCA, HopfieldPottsDCAException
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA

pytestmark = pytest.mark.gpu

U = hc.U
TOY_RNA, TOY_PROTEIN, PF02826 = data_file("toy_rna.fa"), data_file("toy_protein.fa"), data_file("PF02826.faa")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_ctx(X, q, w, kind):
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    if kind == "seqid":
        assert same_bits(ctx.compute_weights(0.8, _lib.DCA_F64), w)       # the reference's weights are the device's
    else:
        ctx.set_weights(w)
    return ctx


def fit_ctx(ctx, a, r, selection=("explicit",)):
    if selection[0] == "likelihood":
        return ctx.mf_hopfield_fit(hc.THETA, num_patterns=selection[1], tol=hc.TOL)
    return ctx.mf_hopfield_fit(hc.THETA, num_attractive=a, num_repulsive=r, tol=hc.TOL)


# ---------------------------------------------------------------- the operator kernel alone
@pytest.mark.parametrize("n", [1, 8, 63, 64, 65, 132, 260, 1100])
def test_operator_kernel_every_element(n):
    """Y = A V against a longdouble product: |dY_rm| <= n 2^-53 sum_k |a_rk| |v_km| (the a priori bound of a sum of n products in
    any order), every element, every block width class; the same bits twice."""
    ctx = _lib.Context(0, _lib.DCA_F64)
    rng = np.random.default_rng(n)
    for b in (1, 9, 16, 17, 72):
        ld = n + 3 if (n, b) in ((65, 17), (1100, 9)) else n               # ld > n, odd: the scalar loads
        A = rng.standard_normal((n, ld))
        A[:, :n] = 0.5 * (A[:, :n] + A[:, :n].T)
        V = rng.standard_normal((n, b))
        Y = ctx.dense_apply(A, V)
        ref = A[:, :n].astype(np.longdouble) @ V.astype(np.longdouble)
        bound = n * U * (np.abs(A[:, :n]) @ np.abs(V))
        ratio = float((np.abs(Y - ref).astype(np.float64) / bound).max())
        print("n", n, "b", b, "ld", ld, "worst error / bound", ratio)
        assert Y.shape == (n, b) and ratio <= 1.0
        assert same_bits(ctx.dense_apply(A, V), Y)
    ctx.close()


def test_operator_kernel_arguments():
    ctx = _lib.Context(0, _lib.DCA_F64)
    for A, V in ((np.zeros((4, 4)), np.zeros((4, 73))), (np.zeros((4, 3)), np.zeros((4, 2)))):
        with pytest.raises(_lib.DcaBackendError) as e:
            ctx.dense_apply(A, V, n=4)
        assert e.value.code == _lib.DCA_ERR_ARG
    ctx.close()


# ---------------------------------------------------------------- one fit, every check
def check_fit(ctx, fit, ref, a, r, what, monkeypatch=None):
    lam, Um, G, T, C_, fi, L, q, n, X = (ref[k] for k in ("lam", "U", "G", "T", "C", "fi", "L", "q", "n", "X"))
    qm, eps = q - 1, ref["eps"]
    idx = href.selected(n, a, r)
    p = len(idx)
    # selection: the same set and the same split
    print(what, "split", fit["num_attractive"], fit["num_repulsive"], "iterations", fit["iterations"], "converged", fit["converged"])
    assert (fit["num_attractive"], fit["num_repulsive"]) == (a, r) and fit["eigenvalues"].shape == (p,)
    assert fit["converged"] == (True, True)
    res = fit["residuals"]
    # eigenvalues: |lambda - lambda_ref| <= r_mu + eps
    dl = np.abs(fit["eigenvalues"] - lam[idx])
    print(what, "eps", eps, "worst |d lambda| / (r + eps)", float((dl / (res + eps)).max()), "largest residual", float(res.max()))
    assert np.all(dl <= res + eps)
    assert np.all(res <= 2.0 * np.array([hc.residual_bound(ref, lam[m]) for m in idx]) + eps)     # converged means what it says
    assert same_bits(fit["gains"], href.gain(fit["eigenvalues"])) or np.abs(fit["gains"] - href.gain(fit["eigenvalues"])).max() <= 4 * U * fit["gains"].max()
    coef = 1.0 - 1.0 / fit["eigenvalues"]
    assert np.array_equal(fit["signs"], np.where(coef < 0, -1, 1))
    # u from the patterns; the residual recomputed against the reference's Gamma
    xi = fit["patterns"].reshape(p, n)
    Ud = (xi / np.sqrt(np.abs(coef))[:, None]).T                    # n x p
    Vd = np.linalg.solve(T, Ud)
    rr = np.linalg.norm(G @ Vd - Vd * fit["eigenvalues"], axis=0)
    print(what, "worst recomputed residual / (r + eps)", float((rr / (res + eps)).max()))
    assert np.all(rr <= res + eps)
    for m in range(p):                                              # the sign rule
        assert Ud[np.argmax(np.abs(Ud[:, m])), m] > 0
    # vectors, where the eigenvalue stands clear: ||u - u_ref||_D <= 2 (r + eps) / gap
    gaps = hc.eigenvalue_gaps(ref)
    compared = hc.compared_patterns(ref, idx)
    assert compared
    D = href.block_diag(href.blocks(C_, L, qm))
    worst = 0.0
    for k in compared:
        d = Ud[:, k] - Um[:, idx[k]]
        dist = float(np.sqrt(d @ D @ d))
        worst = max(worst, dist / (2.0 * (res[k] + eps) / gaps[idx[k]]))
        assert dist <= 2.0 * (res[k] + eps) / gaps[idx[k]], (what, k)
    print(what, "vectors compared", len(compared), "of", p, "worst distance / bound", worst)
    # orthonormality.  Two patterns of one end come out of one orthonormalised block: 8 n 2^-53 plus their residuals, as the
    # issue states it.  A pattern of either end (stated deviation): the two blocks are iterated apart and
    # nothing orthogonalises one against the other, so u_mu^T D u_nu is only what the eigenproblem enforces,
    # (r_mu + r_nu) / |lambda_mu - lambda_nu|; the figure against the literal bound is printed beside it.
    O = np.abs(Ud.T @ D @ Ud - np.eye(p))
    le = fit["eigenvalues"]
    same = (np.arange(p)[:, None] < a) == (np.arange(p)[None, :] < a)
    literal = 8 * n * U + res[:, None] + res[None, :]
    dd = np.abs(le[:, None] - le[None, :]) + np.eye(p)
    obound = np.where(same, literal, 8 * n * U + (res[:, None] + res[None, :]) / dd)
    print(what, "worst |U^T D U - I| / bound: same end", float((O / literal)[same].max()),
          "across the ends", float((O / obound)[~same].max()) if (~same).any() else 0.0,
          "across the ends against the literal bound", float((O / literal)[~same].max()) if (~same).any() else 0.0)
    assert np.all(O <= obound)
    # couplings, every off-diagonal element
    J = ctx.mf_hopfield_couplings()
    assert ctx.mf_model_kind() == _lib.MF_MODEL_HOPFIELD and same_bits(J, J.T)
    Jr = href.couplings(lam, Um, idx)
    mask = href.off_diagonal_mask(L, qm)
    eps_j = ref["eps_couplings"](idx) if "eps_couplings" in ref else href.epsilon(C_, L, qm, idx)["couplings"]
    bound = hc.coupling_bound(ref, idx, res, eps_j)
    print(what, "worst |dJ| / bound", float((np.abs(J - Jr) / bound)[mask].max()), "largest |dJ|", float(np.abs(J - Jr)[mask].max()))
    assert np.all((np.abs(J - Jr) <= bound)[mask])
    # downstream on the installed model: scores and fields of the oracle's functions on the reference J
    blocks = omf.mf_blocks(Jr, L, q)
    fn = omf.frobenius_from_blocks(blocks)
    assert_scores_within(ctx.mf_scores(False), fn, fn)
    assert_scores_within(ctx.mf_scores(True), omf.apc(fn, L), fn)
    if L <= 40:                                                     # every case but PF02826 (18 915 pairs: the oracle's two-site fixed point takes minutes)
        di = omf.direct_info(blocks, fi, L, q)
        assert_scores_within(ctx.mf_di_scores(False), di, di)
        assert_scores_within(ctx.mf_di_scores(True), omf.apc(di, L), di)
    hr = href.fields(Jr, fi, L, q)
    f = np.repeat(fi[:, :qm].reshape(-1)[None, :], n, axis=0) * mask
    hbound = ((bound * f).sum(axis=1) + 8 * n * U * ((np.abs(Jr) * f).sum(axis=1) + np.abs(np.log(fi[:, :qm] / fi[:, qm:])).reshape(-1))).reshape(L, qm)
    h = ctx.mf_fields()
    print(what, "worst field error / bound", float((np.abs(h - hr) / hbound).max()))
    assert np.all(np.abs(h - hr) <= hbound)
    # energies under the reference (J, h)
    Q = X[:9]
    Er = href.energies(Q, Jr, hr, L, q)
    ebound = L * hbound.max() + L * (L - 1) / 2 * bound[mask].max() + 8 * L * L * U * (np.abs(hr).max() * L + np.abs(Jr).max() * L * L)
    E = ctx.mf_energies(Q)
    print(what, "worst energy error / bound", float(np.abs(E - Er).max() / ebound))
    assert np.all(np.abs(E - Er) <= ebound)
    assert same_bits(ctx.mf_sample(6, 3, seed=5), ctx.mf_sample(6, 3, seed=5))
    # overlaps: the contract's chain of doubles; alone, in batches, under pass splits
    rng = np.random.default_rng(7)
    Qs = np.concatenate([X, rng.integers(0, q, size=(70, L), dtype=np.uint8)])[:150]
    want = ctx.hopfield_project(fit["patterns"], Qs)
    oref = href.overlaps(Qs, xi, L, q)
    obnd = L * U * np.abs(fit["patterns"]).max(axis=2).sum(axis=1)            # L 2^-53 sum_i max_a |xi(i, a)|
    print(what, "worst overlap error / bound", float((np.abs(want - oref) / obnd[None, :]).max()))
    assert np.all(np.abs(want - oref) <= obnd[None, :])
    for batch in (1, 7, 64):
        for first in range(0, min(Qs.shape[0], 2 * batch + 1), batch):
            assert same_bits(ctx.hopfield_project(fit["patterns"], Qs[first:first + batch]), want[first:first + batch]), (what, batch, first)
    if monkeypatch is not None:
        monkeypatch.setenv("DCA_NN_PASS", "7")
        assert same_bits(ctx.hopfield_project(fit["patterns"], Qs), want)
        monkeypatch.delenv("DCA_NN_PASS")
    assert same_bits(ctx.hopfield_project(fit["patterns"])[:5], ctx.hopfield_project(fit["patterns"], X[:5]))     # the alignment itself
    return J


@pytest.mark.parametrize("shape, weights", hc.CASES)
def test_planted_alignments(shape, weights, monkeypatch):
    ref = hc.reference(shape, weights)
    a, r = hc.split(shape, weights)
    ctx = make_ctx(ref["X"], ref["q"], ref["w"], weights)
    fit = fit_ctx(ctx, a, r, hc.SELECTION[shape])
    check_fit(ctx, fit, ref, a, r, (shape, weights), monkeypatch)
    ctx.close()


# ---------------------------------------------------------------- the whole spectrum is mfDCA
@pytest.mark.parametrize("shape, a", hc.IDENTITY)
def test_whole_spectrum_equals_mean_field(shape, a, tmp_path):
    """J over the whole spectrum equals -inv(C) off the diagonal blocks: against MeanFieldDCA.get_couplings() of a fresh object,
    within the sum of this fit's bound (hopfield_cases.coupling_bound with nothing unselected) and the inverse's (DESIGN.md
    section 26: 25.52 u |A^-1||A||A^-1|); the same top-L ranking of FN_APC where the reference's score gaps exceed what those
    bounds can move a score."""
    base = hc.reference(shape, "seqid")
    L, q, n = base["L"], base["q"], base["n"]
    qm = q - 1
    letters = "ACGU-" if q == 5 else "ACDEFGHIKLMNPQRSTVWY-"
    path = str(tmp_path / "planted.fa")
    with open(path, "w") as fh:
        for k, row in enumerate(base["X"]):
            fh.write(">s%d\n%s\n" % (k, "".join(letters[c] for c in row)))
    mf = MeanFieldDCA(path, "rna" if q == 5 else "protein", pseudocount=hc.THETA, seqid=0.8)
    Jmf = mf.get_couplings()
    ctx = mf._compare_context()
    assert ctx.mf_model_kind() == _lib.MF_MODEL_MEAN_FIELD
    # the alignment and the weights the class works with (its reader may drop records), and their reference
    X, w, _meff = mf._potts_training()
    C_, fi = href.corr_mat(X, w, q, hc.THETA)
    lam, Um, G, T = href.spectrum(C_, L, qm)
    ref = {"lam": lam, "T": T, "n": n}
    ctx2 = make_ctx(X, q, w, "random")
    fit = fit_ctx(ctx2, a, n - a)
    assert fit["converged"] == (True, True)
    J = ctx2.mf_hopfield_couplings()
    Cinv = np.linalg.inv(C_)
    E = np.abs(Cinv) @ np.abs(C_) @ np.abs(Cinv)
    idx = href.selected(n, a, n - a)
    bound = hc.coupling_bound(ref, idx, fit["residuals"], href.epsilon(C_, L, qm)["couplings"]) + 25.52 * U * E
    mask = href.off_diagonal_mask(L, qm)
    print(shape, a, "iterations", fit["iterations"], "worst |J - J_mf| / bound", float((np.abs(J - Jmf) / bound)[mask].max()),
          "largest |J - J_mf|", float(np.abs(J - Jmf)[mask].max()))
    assert np.all((np.abs(J - Jmf) <= bound)[mask])
    # ranking: a score moves by at most the Frobenius norm of its block's bound (centring is a projection); APC subtracts a
    # product of averages of scores, which moves by at most three times that
    s_h, s_mf = ctx2.mf_scores(True), ctx.mf_scores(True)
    move = 4.0 * float(np.sqrt((omf.mf_blocks(bound * mask, L, q) ** 2).sum(axis=(1, 2))).max())
    order = np.argsort(-s_mf, kind="stable")
    got = np.argsort(-s_h, kind="stable")
    sorted_mf = s_mf[order]
    clear = [t for t in range(min(L, s_mf.size)) if (t == 0 or sorted_mf[t - 1] - sorted_mf[t] > 2.0 * move)
             and (t + 1 == s_mf.size or sorted_mf[t] - sorted_mf[t + 1] > 2.0 * move)]
    print(shape, a, "ranking: positions of the top", L, "clear of the bound:", len(clear))
    assert clear and all(got[t] == order[t] for t in clear)
    ctx2.close()


# ---------------------------------------------------------------- model switching
def test_model_switching_is_bit_exact():
    ref = hc.reference("n60", "random")
    X, q, w = ref["X"], ref["q"], ref["w"]
    ctx, fresh = make_ctx(X, q, w, "random"), make_ctx(X, q, w, "random")
    assert ctx.mf_model_kind() == _lib.MF_MODEL_NONE
    first = ctx.mf_hopfield_fit(hc.THETA, num_patterns=6)
    J1, s1, h1 = ctx.mf_hopfield_couplings(), ctx.mf_scores(True), ctx.mf_fields()
    assert ctx.mf_model_kind() == _lib.MF_MODEL_HOPFIELD
    s_mf, J_mf = ctx.mf_run(hc.THETA, True, want_couplings=True)
    assert ctx.mf_model_kind() == _lib.MF_MODEL_MEAN_FIELD
    s_fresh, J_fresh = fresh.mf_run(hc.THETA, True, want_couplings=True)
    assert same_bits(s_mf, s_fresh) and same_bits(J_mf, J_fresh) and same_bits(ctx.mf_fields(), fresh.mf_fields())
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.mf_hopfield_couplings()                                   # the mean-field model is held: no Hopfield-Potts J to copy
    assert e.value.code == _lib.DCA_ERR_STATE
    second = ctx.mf_hopfield_fit(hc.THETA, num_patterns=6)
    for k in ("eigenvalues", "gains", "signs", "patterns", "residuals"):
        assert same_bits(first[k], second[k]), k
    assert first["iterations"] == second["iterations"]
    assert same_bits(ctx.mf_hopfield_couplings(), J1) and same_bits(ctx.mf_scores(True), s1) and same_bits(ctx.mf_fields(), h1)
    for back in (lambda: ctx.mf_corr_mat(hc.THETA, want=False), lambda: ctx.set_weights(w)):
        ctx.mf_hopfield_fit(hc.THETA, num_attractive=2)
        assert ctx.mf_model_kind() == _lib.MF_MODEL_HOPFIELD
        back()
        assert ctx.mf_model_kind() == _lib.MF_MODEL_NONE
    third = fresh.mf_hopfield_fit(hc.THETA, num_patterns=6)           # another context, after a mean-field run: the same bits
    assert same_bits(third["patterns"], first["patterns"]) and same_bits(fresh.mf_hopfield_couplings(), J1)
    ctx.close()
    fresh.close()


# ---------------------------------------------------------------- errors
def test_errors():
    ref = hc.reference("n8", "random")
    X, q, w = ref["X"], ref["q"], ref["w"]
    ctx = make_ctx(X, q, w, "random")

    def code(**kw):
        with pytest.raises(_lib.DcaBackendError) as e:
            ctx.mf_hopfield_fit(kw.pop("theta", hc.THETA), **kw)
        return e.value.code, str(e.value)
    assert code(num_attractive=5, num_repulsive=4)[0] == _lib.DCA_ERR_ARG            # a + r > n = 8
    assert code(num_attractive=65)[0] == _lib.DCA_ERR_ARG
    assert code(num_repulsive=65)[0] == _lib.DCA_ERR_ARG
    assert code(num_attractive=0, num_repulsive=0)[0] == _lib.DCA_ERR_ARG
    assert code(num_patterns=9)[0] == _lib.DCA_ERR_ARG
    assert code(num_patterns=2, tol=0.0)[0] == _lib.DCA_ERR_ARG
    assert code(num_patterns=2, max_iterations=0)[0] == _lib.DCA_ERR_ARG
    assert ctx.mf_model_kind() == _lib.MF_MODEL_NONE
    ctx.mf_set_row_window(0, 10)
    assert code(num_patterns=2)[0] == _lib.DCA_ERR_STATE
    ctx.mf_set_row_window(0, -1)
    assert ctx.mf_hopfield_fit(hc.THETA, num_patterns=2)["eigenvalues"].shape == (2,)
    # max_iterations reached is reported, not hidden
    big = hc.reference("n140", "random")
    c2 = make_ctx(big["X"], big["q"], big["w"], "random")
    cut = c2.mf_hopfield_fit(hc.THETA, num_attractive=3, num_repulsive=3, max_iterations=2)
    assert cut["iterations"] == (2, 2) and cut["converged"] == (False, False) and cut["residuals"].max() > hc.TOL * big["lam"][0]
    c2.close()
    # a constant column without a pseudocount: the diagonal block of that site is singular
    Xc = X.copy()
    Xc[:, 1] = 2
    c3 = make_ctx(Xc, q, w, "random")
    with pytest.raises(_lib.DcaBackendError) as e:
        c3.mf_hopfield_fit(0.0, num_patterns=2)
    C0, _fi0 = href.corr_mat(Xc, w, q, 0.0)
    singular = [i for i, Dk in enumerate(href.blocks(C0, Xc.shape[1], q - 1)) if np.linalg.eigvalsh(Dk).min() <= 1e-13]
    assert 1 in singular
    assert e.value.code == _lib.DCA_ERR_NOT_SPD and "site %d " % singular[0] in str(e.value)
    c3.close()
    ctx.close()


# ---------------------------------------------------------------- the class and the command line on real alignments
def class_reference(inst, theta):
    X, w, _meff = inst._potts_training()
    q = inst.num_site_states
    L = inst.sequences_len
    C_, fi = href.corr_mat(X, w, q, theta)
    return X, w, q, L, C_, fi


@pytest.mark.parametrize("path, bio, kw", [(TOY_RNA, "rna", dict(num_patterns=6)), (TOY_PROTEIN, "protein", dict(num_attractive=4, num_repulsive=5))],
                         ids=["toy_rna", "toy_protein"])
def test_toy_alignments_through_the_class(path, bio, kw, monkeypatch):
    inst = HopfieldPottsDCA(path, bio, **kw)
    X, w, q, L, C_, fi = class_reference(inst, 0.5)
    lam, Um, G, T = href.spectrum(C_, L, q - 1)
    ref = {"C": C_, "fi": fi, "lam": lam, "U": Um, "G": G, "T": T, "eps": href.MARGIN * href.epsilon(C_, L, q - 1)["eigenvalues"], "L": L,
           "q": q, "n": L * (q - 1), "X": X, "w": w}
    a, r = href.select_likelihood(lam, kw["num_patterns"]) if "num_patterns" in kw else (kw["num_attractive"], kw["num_repulsive"])
    fit = inst.compute_patterns()
    J = check_fit(inst._compare_context(), fit, ref, a, r, os.path.basename(path), monkeypatch)
    assert same_bits(inst.get_couplings(), J)
    # MeanFieldDCA's surface on the Hopfield-Potts couplings
    Jr = href.couplings(lam, Um, href.selected(L * (q - 1), a, r))
    fn = omf.frobenius_from_blocks(omf.mf_blocks(Jr, L, q))
    ranked = inst.compute_sorted_FN_APC()
    assert len(ranked) == L * (L - 1) // 2 and ranked[0][1] >= ranked[-1][1]
    got = np.zeros(len(ranked))
    iu, ju = np.triu_indices(L, k=1)
    where = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(iu, ju))}
    for pair, s in ranked:
        got[where[pair]] = s
    assert_scores_within(got, omf.apc(fn, L), fn)
    assert len(inst.compute_sorted_FN()) == len(inst.compute_sorted_DI()) == len(inst.compute_sorted_DI_APC()) == len(ranked)
    hf = inst.compute_fields()
    assert sorted(hf) == list(range(L)) and np.abs(np.array([hf[i] for i in range(L)]) - href.fields(Jr, fi, L, q)).max() <= 1e-6
    fields, couplings = inst.compute_params(num_site_pairs=3, linear_dist=1)
    assert len(fields) == L and len(couplings) == 3 and couplings[0][1].shape == ((q - 1) ** 2,)
    assert inst._compare_context().mf_model_kind() == _lib.MF_MODEL_HOPFIELD
    # the Potts mixin and the overlaps
    Q = inst._query(None)                                          # every record of the file, duplicates kept
    E = inst.compute_sequence_energies()
    assert E.shape == (Q.shape[0],) and np.isfinite(E).all()
    assert same_bits(inst.sample_sequences(4, num_sweeps=3, seed=2, return_codes=True), inst.sample_sequences(4, num_sweeps=3, seed=2, return_codes=True))
    assert np.isfinite(inst.compute_sequence_pseudo_log_likelihoods()).all()
    ov = inst.project_on_patterns()
    assert ov.shape == (Q.shape[0], a + r) and same_bits(ov, inst._compare_context().hopfield_project(fit["patterns"], Q))
    # another pseudocount: a new fit; a mean-field object never holds the Hopfield-Potts model
    inst(pseudocount=0.3, seqid=0.8)
    assert not same_bits(inst.compute_patterns()["eigenvalues"], fit["eigenvalues"])
    mf = MeanFieldDCA(path, bio)
    mf.compute_sorted_FN_APC()
    assert mf._compare_context().mf_model_kind() == _lib.MF_MODEL_MEAN_FIELD
    with pytest.raises(HopfieldPottsDCAException):
        HopfieldPottsDCA(path, bio)
    with pytest.raises(HopfieldPottsDCAException):
        HopfieldPottsDCA(path, bio, num_attractive=65)


def test_pf02826_both_selections(monkeypatch):
    """The real protein family at p <= 10: the likelihood selection (all attractive on this family) and an explicit (5, 5),
    every check of check_fit on the selected patterns but the DI scores (18 915 pairs in the oracle).  eps comes from the two
    whitenings alone (the unsymmetric third formulation is left out at n = 3900).  The iterations of either end are printed: the
    smallest eigenvalues of a real family cluster, and the repulsive end pays for it."""
    G_ = golden("mf_pf02826")
    inst = HopfieldPottsDCA(PF02826, "protein", num_patterns=10)
    X, w, q, L, C_, fi = class_reference(inst, 0.5)
    assert np.array_equal(X, (G_["X"] - 1).astype(np.uint8))
    n, qm = L * (q - 1), q - 1
    first, second = href.decompose(C_, L, qm, href.whiten_cholesky), href.decompose(C_, L, qm, href.whiten_sqrt)
    lam, Um, G, T, _V = first
    eps = href.epsilon(C_, L, qm, [0], third=False, first=first, second=second)["eigenvalues"]
    ref = {"C": C_, "fi": fi, "lam": lam, "U": Um, "G": G, "T": T, "eps": href.MARGIN * eps, "L": L, "q": q, "n": n, "X": X, "w": w,
           "eps_couplings": lambda idx: href.epsilon(C_, L, qm, idx, third=False, first=first, second=second)["couplings"]}
    for kw in (dict(num_patterns=10), dict(num_attractive=5, num_repulsive=5)):
        obj = inst if "num_patterns" in kw else HopfieldPottsDCA(PF02826, "protein", **kw)
        a, r = href.select_likelihood(lam, 10) if "num_patterns" in kw else (5, 5)
        check_fit(obj._compare_context(), obj.compute_patterns(), ref, a, r, "PF02826 %s" % kw, monkeypatch)
    scores = inst.compute_sorted_FN_APC()
    assert inst._compare_context().mf_model_kind() == _lib.MF_MODEL_HOPFIELD and len(scores) == L * (L - 1) // 2


def test_command_line_writes_its_files(tmp_path):
    out = str(tmp_path / "out")
    text, npy = hopfield_main.run_hopfield_dca(["compute_patterns", "rna", TOY_RNA, "--num_attractive", "3", "--num_repulsive", "2", "--output_dir", out])
    xi = np.load(npy)
    rows = [ln.split() for ln in open(text) if not ln.startswith("#")]
    assert xi.shape == (5, 10, 4) and len(rows) == 5 and [int(r[3]) for r in rows] == [1, 1, 1, -1, -1]
    lam = np.array([float(r[1]) for r in rows])
    assert np.all(lam[:3] > 1) and np.all(lam[3:] < 1) and np.all(np.array([float(r[4]) for r in rows]) < 1e-8)
    assert np.allclose([float(r[2]) for r in rows], href.gain(lam), rtol=1e-14)
    fn = hopfield_main.run_hopfield_dca(["compute_fn", "rna", TOY_RNA, "--num_patterns", "5", "--apc", "--output_dir", out])
    assert os.path.basename(fn) == "HOPFIELD_apc_fn_scores_toy_rna.txt" and len([ln for ln in open(fn) if not ln.startswith("#")]) == 45
    ov = hopfield_main.run_hopfield_dca(["project_sequences", "rna", TOY_RNA, "--num_attractive", "3", "--num_repulsive", "2", "--query_file", TOY_RNA,
                                         "--output_dir", out])
    table = np.array([[float(v) for v in ln.split()[1:]] for ln in open(ov) if not ln.startswith("#")])
    assert table.shape[1] == 5 and table.shape[0] >= 42
    en = hopfield_main.run_hopfield_dca(["compute_energies", "rna", TOY_RNA, "--num_patterns", "5", "--output_dir", out])
    assert os.path.basename(en) == "HOPFIELD_energies_toy_rna.txt"
