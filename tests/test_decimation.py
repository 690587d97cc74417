"""Sparse bmDCA on the GPU (dca_plm_bm_set_mask / get_mask / decimate, dca_plm_zero_sum_gauge, PlmDCA.decimate_boltzmann, plmdca
decimate_boltzmann) against the numpy restatements of tests/decimation_reference.py and tests/test_boltzmann.py.  The shapes
meet the pair-tile sizes of bm_tile that a plm model can have (dca_plm_configure takes q = 5 and q = 21 only: TB = 16 and
TB = 4; the TB = 2 tile of q > 24 is reached by the counting entries alone), each with a ragged last tile, at 70 chains (not a
multiple of 64), in both storage precisions."""
import os

import numpy as np
import pytest

import decimation_reference as ref
from conftest import data_file
from pydca_amd import _lib, plmdca_main
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from test_boltzmann import bm_context, bm_ref, data_stats, model_stats, record
from test_potts_sampling import gibbs_ref, plm_model

pytestmark = pytest.mark.gpu

SHAPES = [(17, 5), (6, 21)]                              # (L, q): TB = 16 and TB = 4
PRECS = [_lib.DCA_F32, _lib.DCA_F64]
N, K, E, SEED, LAM = 70, 2, 1, 19, 0.02
RATES = (0.3, 0.2, 0.01, 0.02)
U = 2.0 ** -53


def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def begin(ctx, n=N, seed=SEED):
    ctx.plm_bm_begin(n, K, E, seed=seed, eta_h=RATES[0], eta_J=RATES[1], mu_h=RATES[2], mu_J=RATES[3], pseudocount=LAM)


def started(L, q, prec, iterations=2):
    """a context after begin and `iterations` iterations -> (ctx, X, dtype, x before begin)"""
    ctx, X, dt = bm_context(L, q, prec, 10 * q + prec)
    x0 = ctx.plm_get_x(dt)
    begin(ctx)
    ctx.plm_bm_iterate(iterations)
    return ctx, X, dt, x0


def couplings(x, L, q):
    return x[L * q:].reshape(-1, q, q)


# ---------------------------------------------------------------- 1. score per element
@pytest.mark.parametrize("L,q", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_score_per_element(L, q, prec):
    """Relative bound: c * u / min(p, 1 - p) with c = 4 x the largest ratio the float64 numpy restatement itself reaches against
    longdouble on the same inputs (the device's expm1 and division may round differently from libm's)."""
    ctx, X, dt, _x0 = started(L, q, prec)
    x = ctx.plm_get_x(dt)
    mask0 = ctx.plm_bm_get_mask()
    _gi, gij = ctx.plm_bm_freqs(1)
    info = ctx.plm_bm_decimate(0, return_scores=True)
    D = info["scores"]
    J = couplings(x, L, q).astype(np.float64)
    want = ref.score(J, gij, np.longdouble)
    host = ref.score(J, gij, np.float64)
    live = want > 0
    assert live.any() and np.array_equal(D == 0, ~live) and not np.any(np.signbit(D))
    cond = 1.0 / np.minimum(gij[live], 1.0 - gij[live])
    unit = U * cond * want[live]
    c_host = float(np.max(np.abs(host[live] - want[live]) / unit))
    c_dev = float(np.max(np.abs(D[live] - want[live]) / unit))
    print("score ratios (L %d, q %d, f%d): numpy float64 %.4f, device %.4f" % (L, q, prec, c_host, c_dev))
    assert c_dev <= 4.0 * c_host, (c_host, c_dev)
    assert info["active_before"] == info["active_after"] == D.size and info["removed"] == 0
    assert ctx.plm_get_x(dt).tobytes() == x.tobytes()                  # remove = 0 touches nothing
    assert np.array_equal(ctx.plm_bm_get_mask(), mask0) and mask0.all()
    ctx.close()


# ---------------------------------------------------------------- 2. the selection is exact
@pytest.mark.parametrize("L,q,prec", [(L, q, p) for L, q in SHAPES for p in PRECS] + [(70, 21, _lib.DCA_F32)])
def test_selection_is_exact(L, q, prec):
    """(70, 21): 260 chunks of the count and apply passes, so the scan gives a thread two entries and the tie group at D = 0
    runs across many workgroups"""
    ctx, X, dt = bm_context(L, q, prec, 10 * q + prec)
    x0 = ctx.plm_get_x(dt)
    total = L * (L - 1) // 2 * q * q
    zeros = None
    for pick in ("one", "inside", "past", "all"):
        ctx.plm_set_x(x0)
        begin(ctx)                                                     # a new run: no mask, the same chains
        ctx.plm_bm_iterate(2)
        x = ctx.plm_get_x(dt)
        if zeros is None:
            zeros = int((ctx.plm_bm_decimate(0, return_scores=True)["scores"] == 0).sum())
            assert zeros >= 2, "the tie group at D = 0 must not be empty"
        remove = dict(one=1, inside=zeros // 2, past=zeros + 1, all=total)[pick]
        info = ctx.plm_bm_decimate(remove, return_scores=True)
        D = info.pop("scores")
        gone = np.flatnonzero(ctx.plm_bm_get_mask().ravel() == 0)
        assert np.array_equal(gone, ref.select(D, remove)), pick
        want = ref.selection_info(D, remove)
        assert info["active_before"] == total and info["removed"] == remove and info["active_after"] == total - remove
        assert np.float64(info["threshold"]).tobytes() == np.float64(want["threshold"]).tobytes(), pick
        assert np.float64(info["removed_sum"]).tobytes() == np.float64(want["removed_sum"]).tobytes(), pick
        y = ctx.plm_get_x(dt)
        assert y[:L * q].tobytes() == x[:L * q].tobytes()
        Jx, Jy = x[L * q:], y[L * q:]
        keep = np.ones(total, dtype=bool)
        keep[gone] = False
        assert Jy[keep].tobytes() == Jx[keep].tobytes()
        assert np.all(Jy[gone] == 0) and not np.any(np.signbit(Jy[gone]))
    ctx.close()


# ---------------------------------------------------------------- 3. the mask holds
@pytest.mark.parametrize("L,q", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_mask_holds_through_iterations(L, q, prec):
    ctx, X, dt, x0 = started(L, q, prec)
    fi, fij = data_stats(X, np.ones(X.shape[0]), q, LAM)
    S, xr, _gi, _gij, _rec = bm_ref(x0, fi, fij, N, K, E, 2, SEED, RATES)[-1]
    assert ctx.plm_get_x(dt).tobytes() == xr.tobytes()
    total = L * (L - 1) // 2 * q * q
    first = ctx.plm_bm_decimate(total // 3)
    mask = ctx.plm_bm_get_mask().astype(bool)
    assert int((~mask).sum()) == total // 3
    xr = xr.copy()
    xr[L * q:][~mask.ravel()] = 0
    assert ctx.plm_get_x(dt).tobytes() == xr.tobytes()
    chains = np.arange(N)
    for t in range(2, 5):
        rec = ctx.plm_bm_iterate(1)[0]
        h, Jp = plm_model(xr, L, q)
        S, m = gibbs_ref(h, Jp, 1.0, SEED, chains, E + t * K, K, S)
        assert m > 1e-12
        gi, gij = model_stats(S, q)
        want = record(fi, fij, gi, gij, L)
        xr = ref.masked_update(xr, fi, fij, gi, gij, RATES, mask)
        assert np.array_equal(ctx.plm_bm_chains(), S), t
        y = ctx.plm_get_x(dt)
        assert y.tobytes() == xr.tobytes(), t
        gone = y[L * q:][~mask.ravel()]
        assert np.all(gone == 0) and not np.any(np.signbit(gone)), t
        assert rec[:2].tobytes() == want[:2].tobytes(), (t, rec, want)
        assert abs(rec[2] - want[2]) <= 1e-12, (t, rec, want)
    second = ctx.plm_bm_decimate(total // 4, return_scores=True)
    assert np.all(second["scores"][~mask] == -1.0) and np.all(second["scores"][mask] >= 0)
    mask2 = ctx.plm_bm_get_mask().astype(bool)
    assert not np.any(mask2 & ~mask)                                   # only active elements were drawn
    assert second["active_before"] == first["active_after"] == total - total // 3
    assert second["active_after"] == int(mask2.sum()) == total - total // 3 - total // 4
    ctx.close()


# ---------------------------------------------------------------- 4. an all-ones mask is the unmasked run
@pytest.mark.parametrize("prec", PRECS)
def test_all_ones_mask_is_the_unmasked_run(prec):
    L, q, T = 6, 21, 3
    runs = []
    for masked in (False, True):
        ctx, X, dt = bm_context(L, q, prec, 10 * q + prec)
        begin(ctx)
        if masked:
            ctx.plm_bm_set_mask(np.ones((L * (L - 1) // 2, q, q), dtype=np.uint8))
        recs = ctx.plm_bm_iterate(T)
        runs.append((ctx.plm_get_x(dt), recs, ctx.plm_bm_chains()))
        if masked:
            rng = np.random.default_rng(8)
            planted = (rng.random((L * (L - 1) // 2, q, q)) < 0.6).astype(np.uint8)
            x = ctx.plm_get_x(dt)
            ctx.plm_bm_set_mask(planted)
            assert np.array_equal(ctx.plm_bm_get_mask(), planted)
            y = ctx.plm_get_x(dt)
            want = x.copy()
            want[L * q:][planted.ravel() == 0] = 0
            assert y.tobytes() == want.tobytes()
            assert ctx.plm_bm_decimate(0)["active_before"] == int(planted.sum())
        ctx.close()
    (xa, ra, ca), (xb, rb, cb) = runs
    assert xa.tobytes() == xb.tobytes() and ra.tobytes() == rb.tobytes() and np.array_equal(ca, cb)


# ---------------------------------------------------------------- 5. the gauge on the device
@pytest.mark.parametrize("L,q", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_gauge_on_the_device(L, q, prec):
    ctx, X, dt = bm_context(L, q, prec, 10 * q + prec)
    x = ctx.plm_get_x(dt)
    Q = np.random.default_rng(6).integers(0, q, size=(20, L), dtype=np.uint8)
    E0 = ctx.plm_energies(Q)
    ctx.plm_zero_sum_gauge()
    y = ctx.plm_get_x(dt)
    want, mag = ref.zero_sum_gauge(x.astype(np.float64), L, q, details=True)     # float64 result of the stored values
    if prec == _lib.DCA_F64:
        assert y.tobytes() == want.tobytes()
    else:
        assert np.all(np.abs(y.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -149)
    # Every bound is (number of terms + 8) u sum |term| in float64, the terms and their magnitudes from the reference.  Float32
    # storage adds the one rounding of every stored value of the new model, s = 2^-24 times their magnitudes; nothing else.
    s32 = 0.0 if prec == _lib.DCA_F64 else 2.0 ** -24
    # energies shift by one constant: four energies of nt = L + pairs terms each enter shift[k] - shift[0]
    nt = L + L * (L - 1) // 2
    shift = ctx.plm_energies(Q) - E0
    _e, m0 = ref.energies(x, Q, L, q)
    _e, m1 = ref.energies(want, Q, L, q)
    bound = (nt + 8) * U * (m0 + m1 + m0[0] + m1[0]) + s32 * (m1 + m1[0])
    assert np.all(np.abs(shift - shift[0]) <= bound), (np.max(np.abs(shift - shift[0]) / bound))
    # block rows and columns: 4 q addends each (J, r, c, m)
    Jy, Jw = couplings(y, L, q).astype(np.float64), np.abs(couplings(want, L, q))
    assert np.all(np.abs(Jy.sum(axis=2)) <= (4 * q + 8) * U * mag["row"] + s32 * Jw.sum(axis=2))
    assert np.all(np.abs(Jy.sum(axis=1)) <= (4 * q + 8) * U * mag["col"] + s32 * Jw.sum(axis=1))
    # a site's fields: q (L + 1) addends (h, the L - 1 parts, u)
    hy, hw = y[:L * q].astype(np.float64).reshape(L, q), np.abs(want[:L * q]).reshape(L, q)
    assert np.all(np.abs(hy.sum(axis=1)) <= (q * (L + 1) + 8) * U * mag["site"] + s32 * hw.sum(axis=1))
    begin(ctx)
    ctx.plm_zero_sum_gauge()                                           # a run without removed elements allows it
    ctx.plm_bm_iterate(1)
    ctx.plm_zero_sum_gauge()
    ctx.plm_bm_decimate(3)
    assert _code(ctx.plm_zero_sum_gauge) == _lib.DCA_ERR_STATE
    ctx.plm_bm_end()
    ctx.plm_zero_sum_gauge()
    ctx.close()


# ---------------------------------------------------------------- 6. states and arguments
@pytest.mark.parametrize("L,q", [(3, 25), (5, 2)])
def test_other_alphabets_have_no_plm_model(L, q):
    """q = 25 (TB = 2) and q = 2 never reach the decimation: the plm engine refuses them at dca_plm_configure"""
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(np.random.default_rng(q).integers(0, q, size=(20, L), dtype=np.uint8), q)
    ctx.set_weights(np.ones(20))
    assert _code(lambda: ctx.plm_configure(1.0, 1.0)) == _lib.DCA_ERR_ARG
    assert _code(ctx.plm_zero_sum_gauge) == _lib.DCA_ERR_STATE
    ctx.close()


def test_states_and_arguments():
    L, q = 6, 21
    total = L * (L - 1) // 2 * q * q
    ctx, X, dt = bm_context(L, q, _lib.DCA_F32, 4)
    ones = np.ones(total, dtype=np.uint8)
    assert _code(lambda: ctx.plm_bm_decimate(1)) == _lib.DCA_ERR_STATE          # no run
    assert _code(lambda: ctx.plm_bm_set_mask(ones)) == _lib.DCA_ERR_STATE
    assert _code(ctx.plm_bm_get_mask) == _lib.DCA_ERR_STATE
    begin(ctx)
    assert _code(lambda: ctx.plm_bm_decimate(1)) == _lib.DCA_ERR_STATE          # no iteration yet
    ctx.plm_bm_iterate(1)
    assert _code(lambda: ctx.plm_bm_decimate(-1)) == _lib.DCA_ERR_ARG
    assert _code(lambda: ctx.plm_bm_decimate(total + 1)) == _lib.DCA_ERR_ARG
    bad = ones.copy()
    bad[17] = 2
    assert _code(lambda: ctx.plm_bm_set_mask(bad)) == _lib.DCA_ERR_ARG
    assert _lib.lib().dca_plm_bm_set_mask(ctx._h, None) == _lib.DCA_ERR_ARG
    assert _lib.lib().dca_plm_bm_get_mask(ctx._h, None) == _lib.DCA_ERR_ARG
    ctx.set_profiling(True)
    ctx.plm_bm_decimate(10)
    assert ctx.kernel_time("bm_decimate")[1] == 1
    assert _code(lambda: ctx.plm_bm_decimate(total - 9)) == _lib.DCA_ERR_ARG    # more than the active elements
    assert int(ctx.plm_bm_get_mask().sum()) == total - 10
    ctx.plm_bm_end()
    begin(ctx)
    assert ctx.plm_bm_get_mask().all()                                           # a mask ends with its run
    ctx.plm_bm_iterate(1)
    ctx.plm_bm_decimate(5)
    begin(ctx)                                                                   # ... and with a new begin
    assert ctx.plm_bm_get_mask().all()
    ctx.close()


# ---------------------------------------------------------------- 7. determinism
def test_decimation_is_deterministic():
    L, q = 17, 5
    out = []
    for _ in range(2):
        ctx, X, dt, _x0 = started(L, q, _lib.DCA_F32)
        info = ctx.plm_bm_decimate(1234, return_scores=True)
        out.append((ctx.plm_bm_get_mask(), ctx.plm_get_x(dt), info))
        ctx.close()
    (ma, xa, ia), (mb, xb, ib) = out
    assert np.array_equal(ma, mb) and xa.tobytes() == xb.tobytes()
    assert ia["scores"].tobytes() == ib["scores"].tobytes()
    for k in ("active_before", "removed", "active_after", "threshold", "removed_sum"):
        assert np.float64(ia[k]).tobytes() == np.float64(ib[k]).tobytes(), k


# ---------------------------------------------------------------- 8. class and command line
def test_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    kw = dict(target_density=0.3, drop_fraction=0.2, num_chains=128, warmup_iterations=20, max_iterations_per_round=10)
    fits = []
    for _ in range(2):
        inst = PlmDCA(path, "protein", max_iterations=5)
        fits.append(inst.decimate_boltzmann(**kw))
    fit = fits[0]
    L, q = inst.sequences_len, 21
    pairs = L * (L - 1) // 2
    x, mask = fit["fields_and_couplings"], fit["mask"]
    assert mask.shape == (pairs, q, q) and mask.dtype == np.bool_ and x.dtype == np.float32
    target = int(round(0.3 * pairs * q * q))
    assert int(mask.sum()) == target and fit["density"] == mask.mean() == target / float(pairs * q * q)
    J = couplings(x, L, q)
    assert np.all(J[~mask] == 0) and np.any(J[mask] != 0)
    R, H = fit["rounds"], fit["history"]
    assert R.shape[1] == 6 and H.shape[1] == 3 and H.shape[0] >= R[-1, 0]
    assert R[0, 1] == pairs * q * q and np.all(R[1:, 1] == R[:-1, 1] - R[:-1, 2]) and R[-1, 1] - R[-1, 2] == target
    assert np.all(np.diff(R[:, 0]) > 0) and np.all(np.diff(R[:, 3]) < 0) and R[-1, 3] == fit["density"]
    seqs = ["VDQSSWD-", "PQYYDKVK", "SDWTVKDC"]
    codes = _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_PROTEIN, L, 0)
    want, _mag = ref.energies(x, codes, L, q)
    assert np.allclose(inst.compute_sequence_energies(seqs), want, rtol=1e-12, atol=1e-12)
    for k in ("history", "rounds", "mask", "fields_and_couplings"):
        assert np.asarray(fits[0][k]).tobytes() == np.asarray(fits[1][k]).tobytes(), k
    with pytest.raises(PlmDCAException):
        PlmDCA(path, "protein", devices=[0, 1]).decimate_boltzmann(**kw)
    out = str(tmp_path / "dec_out")
    files = plmdca_main.run_plm_dca(["decimate_boltzmann", "protein", path, "--max_iterations", "5", "--output_dir", out,
                                     "--target_density", "0.3", "--drop_fraction", "0.2", "--num_chains", "128",
                                     "--warmup_iterations", "20", "--max_iterations_per_round", "10", "--num_samples", "5",
                                     "--num_sweeps", "3"])
    assert [os.path.basename(f) for f in files] == ["PLMDCA_decimation_toy_protein.txt", "PLMDCA_decimation_params_toy_protein.npy",
                                                    "PLMDCA_decimation_mask_toy_protein.npy", "PLMDCA_decimation_samples_toy_protein.fa"]
    params, m = np.load(files[1]), np.load(files[2])
    assert params.tobytes() == x.tobytes() and np.array_equal(m, mask)
    assert np.all(couplings(params, L, q)[~m] == 0)
    rows = [ln.split() for ln in open(files[0]).read().splitlines() if not ln.startswith("#")]
    assert len(rows) == R.shape[0] and all(len(r) == 6 for r in rows)
