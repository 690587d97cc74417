"""The element audit of the fitted Potts model as a sequence model on the GPU: energies and the single-mutant scan, PLL / site /
cond, plain Gibbs sweeps, AIS and bmDCA iterations through _lib.Context for the three model sources (plm float32, plm float64,
mf), over the case table of tests/potts_audit_reference.py, which reaches every tile size, accumulator count, chunking and LDS
layout the kernels pick from (q, element size, L).  Every value the device returns is held to a longdouble reference within a
derived bound, every chain to the restatement's codes; tests/test_potts_audit_host.py pins the table, the bounds and the audit
functions on the CPU.  Each test prints its worst error over bound (pytest -s)."""
import numpy as np
import pytest

import potts_audit_reference as R
from pydca_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("pottsplan"))


class Model:
    """a context that holds the case's model, the model as the reference reads it, and the entries of its source"""
    def __init__(self, case, sigma, N=40):
        self.case = case
        L, q = case.L, case.q
        if case.src == "mf":
            X, w = R.mf_alignment(case)
            self.ctx = ctx = _lib.Context(0, _lib.DCA_F64)
            ctx.set_msa(X, q)
            if w is None:
                ctx.compute_weights(0.8, _lib.DCA_F64)
            else:
                ctx.set_weights(w)
            ctx.mf_corr_mat(R.MF.THETA, want=False)
            self.h, self.Jp = (R.mf_model_lazy if case.device_model_only else R.mf_model)(ctx.mf_couplings(), ctx.mf_fields(), L, q)
            self.energies, self.scan, self.pll, self.sample, self.ais = (ctx.mf_energies, ctx.mf_mutation_scan, ctx.mf_pseudo_likelihood,
                                                                        ctx.mf_sample, ctx.mf_ais)
        else:
            prec = _lib.DCA_F32 if case.src == "f32" else _lib.DCA_F64
            self.X = R.training_alignment(case, N)
            self.ctx = ctx = _lib.Context(0, prec)
            ctx.set_msa(self.X, q)
            ctx.set_weights(np.ones(N))
            ctx.plm_configure(1.0, 1.0)
            self.x = R.plm_x(case.name, sigma)
            ctx.plm_set_x(self.x)
            assert ctx.plm_get_x(case.dtype.type).tobytes() == self.x.tobytes()        # the reference sees the stored values
            self.h, self.Jp = R.model_of(case, sigma)
            self.energies, self.scan, self.pll, self.sample, self.ais = (ctx.plm_energies, ctx.plm_mutation_scan, ctx.plm_pseudo_likelihood,
                                                                        ctx.plm_sample, ctx.plm_ais)

    def close(self):
        self.ctx.close()


def report(case, *audits, extra=""):
    print("\n%s: %s%s" % (case.name, "; ".join(a.summary() for a in audits), extra))
    R.assert_ok(*audits)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------- energies and the scan
@pytest.mark.parametrize("case", R.cases_of("energy"), ids=lambda c: c.name)
def test_energies_and_scan(driver, case):
    plan = R.plan_of(case, driver)
    m = Model(case, R.SIGMA_PLL)
    X = R.queries(case, 32 if case.L > 131 else R.N_QUERIES)
    assert np.any(X == case.q - 1)                                   # kind 1's gap state is read
    E = m.energies(X)
    w = X[3 % len(X)]
    dE = m.scan(w)
    m.close()
    a = R.audit_energies(R.energy_reference(m.h, m.Jp, X, plan["G"]), E)
    b = R.audit_scan(R.scan_reference(m.h, m.Jp, w), dE)
    assert a.checked == len(X) and b.checked == case.L * case.q
    report(case, a, b)


def test_energies_across_the_sequence_blocks():
    """n = 4097 at q 5, L 9: a second block of 4096 sequences (blockIdx.y = 1) with one sequence; the last 4095, 4096 and 1 scored
    alone have the same bits"""
    case = R.BY_NAME["q5_L9_f32"]
    m = Model(case, R.SIGMA_PLL)
    X = R.queries(case, 4097)
    E = m.energies(X)
    for n in (4095, 4096, 1):
        assert np.array_equal(bits(m.energies(X[-n:])), bits(E[-n:])), n
    m.close()
    report(case, R.audit_energies(R.energy_reference(m.h, m.Jp, X, 1), E))


def test_energies_across_the_passes():
    """n = 65537 at q 2, L 2: the second pass of kEChunk = 65536 queries holds one sequence"""
    case = R.BY_NAME["q2_L2_mf"]
    m = Model(case, R.SIGMA_PLL)
    X = R.queries(case, 65537)
    E = m.energies(X)
    m.close()
    states = np.array([[a, b] for a in range(2) for b in range(2)], dtype=np.uint8)
    ref = R.energy_reference(m.h, m.Jp, states, 1)
    code = X[:, 0].astype(np.int64) * 2 + X[:, 1]
    assert len(np.unique(code)) == 4
    ref.E, ref.bound = ref.E[code], ref.bound[code]
    report(case, R.audit_energies(ref, E))
    assert np.array_equal(bits(E[65536:]), bits(E[:65536][code[:65536] == code[65536]][:1]))      # the same bits as in the first pass


# ----------------------------------------------------------------------------- PLL, site, cond
@pytest.mark.parametrize("case", R.cases_of("pll"), ids=lambda c: c.name)
def test_conditionals(case):
    m = Model(case, R.SIGMA_PLL)
    X = R.queries(case, 16 if case.L > 131 else R.N_QUERIES)
    assert np.any(X == case.q - 1)                                   # kind 1's gap state is read
    pll, site, cond = m.pll(X, per_site=True, conditionals=True)
    m.close()
    ref = R.cond_reference(m.h, m.Jp, X)
    audits = R.audit_conditionals(ref, pll, site, cond)
    assert audits[0].checked == X.size * case.q
    report(case, *audits, extra="; exp %.3f ulps, log %.3f ulps" % (ref.exp_ulps, ref.log_ulps))


def test_conditionals_across_the_passes(monkeypatch):
    """DCA_PLL_PASS = 512 and n = 513: a second pass with one query, at QM 32"""
    case = R.BY_NAME["q25_L11_mf"]
    m = Model(case, R.SIGMA_PLL)
    X = R.queries(case, 513)
    one = m.pll(X, per_site=True, conditionals=True)
    monkeypatch.setenv("DCA_PLL_PASS", "512")
    two = m.pll(X, per_site=True, conditionals=True)
    m.close()
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()
    report(case, *R.audit_conditionals(R.cond_reference(m.h, m.Jp, X[500:]), *[v[500:] for v in two]))


# ----------------------------------------------------------------------------- plain sweeps
@pytest.mark.parametrize("case", R.cases_of("sample"), ids=lambda c: c.name)
def test_plain_sweeps(case):
    m = Model(case, R.SIGMA_SAMPLE)
    runs = R.sample_reference(case, m.h, m.Jp)                       # asserts the margin condition of every draw
    audits = []
    for beta, X0, c0, s0, seed, codes, margin in runs:
        out = m.sample(case.chains, case.sweeps, seed=seed, beta=beta, initial=X0, first_chain=c0, first_sweep=s0)
        audits.append(R.audit_codes("beta %g %s start" % (beta, "drawn" if X0 is None else "given"), codes, out))
    m.close()
    report(case, *audits, extra="; smallest draw margin %.3g" % min(r[-1] for r in runs))


def test_chains_do_not_depend_on_their_number():
    """n = 63, 64 and 65 chains: chain c has the same codes in each"""
    case = R.BY_NAME["q21_L20_f32"]
    m = Model(case, R.SIGMA_SAMPLE)
    outs = {n: m.sample(n, 2, seed=9, beta=1.0) for n in (63, 64, 65)}
    m.close()
    assert np.array_equal(outs[63], outs[65][:63]) and np.array_equal(outs[64], outs[65][:64])
    codes, margin = R.gibbs_ref(m.h, m.Jp, 1.0, 9, np.arange(65), 0, 2, R.random_start(9, np.arange(65), case.L, case.q))
    R.assert_margin(case, margin, 1.0, R.model_sabs(m.h, m.Jp))
    report(case, R.audit_codes("65 chains", codes, outs[65]))


# ----------------------------------------------------------------------------- AIS
@pytest.mark.parametrize("case", R.cases_of("ais"), ids=lambda c: c.name)
def test_ais(driver, case):
    plan = R.plan_of(case, driver)
    m = Model(case, R.SIGMA_SAMPLE)
    audits, margins = [], []
    for k, run in enumerate(R.ais_runs(case)):
        ref = R.ais_reference(case, m.h, m.Jp, plan["G"], run, k)
        a = ref.args
        logw, lz0, X = m.ais(case.chains, a["K"], sweeps_per_temperature=a["s"], seed=a["seed"], first_chain=a["first_chain"],
                             betas=a["betas"], base_fields=a["base_fields"], return_chains=True)
        audits += list(R.audit_ais(ref, logw, X))
        margins.append(ref.margin)
        assert abs(lz0 - ref.lz0) <= 1e-12 * abs(ref.lz0)
    m.close()
    report(case, *audits, extra="; smallest draw margin %.3g" % min(margins))


# ----------------------------------------------------------------------------- bmDCA
@pytest.mark.parametrize("case", R.cases_of("bm"), ids=lambda c: c.name)
def test_bm_iterations(case):
    m = Model(case, R.SIGMA_SAMPLE, N=60)
    ctx, n = m.ctx, case.chains
    fi, fij, want = R.bm_reference(case, m.x, m.X)
    eh, eJ, mh, mJ = R.BM_RATES
    seed = R.seed_of(case, 90)
    ctx.plm_bm_begin(n, R.BM_K, R.BM_E, seed=seed, eta_h=eh, eta_J=eJ, mu_h=mh, mu_J=mJ, pseudocount=R.BM_LAMBDA)
    dfi, dfij = ctx.plm_bm_freqs(0)
    assert dfi.tobytes() == fi.tobytes() and dfij.tobytes() == fij.tobytes()
    audits = []
    for t in range(R.BM_T):
        rec = ctx.plm_bm_iterate(1)[0]
        gi, gij = ctx.plm_bm_freqs(1)
        audits.append(R.audit_bm("iteration %d" % t, want[t], (ctx.plm_bm_chains(), ctx.plm_get_x(case.dtype.type), gi, gij, rec)))
    ctx.plm_bm_end()
    # the zero-rate form: x untouched, the chains are the sampler's, the counts theirs
    ctx.plm_set_x(m.x)
    ctx.plm_bm_begin(n, R.BM_K, R.BM_E, seed=seed, mu_h=0.3, mu_J=0.2, pseudocount=R.BM_LAMBDA)
    rec = ctx.plm_bm_iterate(1)[0]
    gi, gij = ctx.plm_bm_freqs(1)
    S = want[0][0]
    audits.append(R.audit_bm("zero rates", (S, m.x, want[0][2], want[0][3], want[0][4]),
                             (ctx.plm_bm_chains(), ctx.plm_get_x(case.dtype.type), gi, gij, rec)))
    ctx.plm_bm_end()
    m.close()
    report(case, *audits)
