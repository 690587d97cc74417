"""Host side of conditional Gibbs sampling (dca_plm_sample_conditional, dca_mf_sample_conditional): the
exported entries, the argument checks of sample_sequences_conditional, the site-range parser, the sample_conditional
sub-command, and the masked float64 numpy restatement the GPU tests compare with (test_conditional_sampling.py), held here to
the plain sampler's restatement.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.fasta_reader import fasta_reader  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCAException  # noqa: E402
from test_potts_sampling import gibbs_ref, random_start, uniforms  # noqa: E402

ENTRIES = ("dca_plm_sample_conditional", "dca_mf_sample_conditional")
TOY_RNA = os.path.join(ROOT, "tests", "data", "toy_rna.fa")


# ---------------------------------------------------------------- the masked restatement
def pair_lookup(L):
    iu, ju = np.triu_indices(L, 1)
    pidx = np.zeros((L, L), dtype=np.int64)
    pidx[iu, ju] = np.arange(iu.size)
    pidx[ju, iu] = np.arange(iu.size)
    return pidx


def row_blocks(Jp, pidx, i, sites):
    """B[k][a, b] = J_ij(a, b) for j = sites[k] (j != i)"""
    sites = np.asarray(sites, dtype=np.int64)
    B = np.asarray(Jp[pidx[i, sites]], dtype=np.float64).copy()
    below = sites < i
    B[below] = B[below].transpose(0, 2, 1)                      # j < i: J(a, b) = block(j, i)[b, a]
    return B


def terms(B, codes):
    """T[k, n, a] = B[k][a, codes[n, k]]"""
    K = B.shape[0]
    return B[np.arange(K)[:, None], :, codes.T]


def sequential(start, T):
    """start + T[0] + T[1] + ... one term after another (cumsum keeps the order)"""
    return np.cumsum(np.concatenate([start[None], T], axis=0), axis=0)[-1] if T.shape[0] else start


def draw(u, beta, U):
    """the samplers' rule -> (picks, smallest |cum - r| / T)"""
    q = u.shape[1]
    p = np.exp(beta * (u - u.max(axis=1, keepdims=True)))
    cum = np.cumsum(p, axis=1)
    T = cum[:, -1]
    r = U * T
    above = cum > r[:, None]
    pick = np.where(above.any(axis=1), above.argmax(axis=1), q - 1 - np.argmax((p > 0)[:, ::-1], axis=1))
    return pick, float((np.abs(cum - r[:, None]) / T[:, None]).min())


def cond_gibbs_ref(h, Jp, beta, seed, chains, first_sweep, sweeps, X0, free, randomize):
    """The specification in float64: c_i = h_i + the clamped terms (j ascending, one by one); per sweep and free position kappa
    u = (((c + S_0) + S_1) + S_2) + S_3 with S_0's terms joining c one by one and S_1 .. S_3 summed from 0, positions k = w
    (mod 4), k != kappa, ascending; Philox counters carry the site index.  -> (codes, smallest relative draw margin)."""
    L, q = h.shape
    free = np.asarray(free, dtype=np.int64)
    F = free.size
    clamped = np.setdiff1d(np.arange(L), free)
    S = np.asarray(X0).astype(np.int64).copy()
    n = S.shape[0]
    if randomize:
        for i in free:
            S[:, i] = np.floor(uniforms(seed, chains, 0, int(i), 1) * q).astype(np.int64)
    pidx = pair_lookup(L)
    margin = np.inf
    if sweeps == 0 or F == 0:
        return S.astype(np.uint8), margin
    fields, blocks = [], []
    for i in free:
        c = np.repeat(h[i][None, :].astype(np.float64), n, axis=0)
        fields.append(sequential(c, terms(row_blocks(Jp, pidx, i, clamped), S[:, clamped])))
        blocks.append(row_blocks(Jp, pidx, i, free))
    for t in range(sweeps):
        for kappa, i in enumerate(free):
            u = None
            for w in range(4):
                ks = np.array([k for k in range(w, F, 4) if k != kappa], dtype=np.int64)
                T = terms(blocks[kappa][ks], S[:, free[ks]]) if ks.size else np.zeros((0, n, q))
                part = sequential(fields[kappa] if w == 0 else np.zeros((n, q)), T)
                u = part if w == 0 else u + part
            pick, m = draw(u, beta, uniforms(seed, chains, first_sweep + t, int(i), 0))
            margin = min(margin, m)
            S[:, i] = pick
    return S.astype(np.uint8), margin


def masked_plain_ref(h, Jp, beta, seed, chains, first_sweep, sweeps, X0, free, randomize):
    """An independent statement: gibbs_ref's site sum over ALL j != i (numpy's own order), only the free sites visited."""
    L, q = h.shape
    S = np.asarray(X0).astype(np.int64).copy()
    if randomize:
        R = random_start(seed, chains, L, q)
        S[:, free] = R[:, free]
    pidx = pair_lookup(L)
    others = np.arange(L)
    for t in range(sweeps):
        for i in free:
            js = others[others != i]
            u = h[i][None, :] + terms(row_blocks(Jp, pidx, i, js), S[:, js]).sum(axis=0)
            S[:, i], _m = draw(u, beta, uniforms(seed, chains, first_sweep + t, int(i), 0))
    return S.astype(np.uint8)


def random_model(L, q, seed, sigma=0.5):
    rng = np.random.default_rng(seed)
    return rng.normal(0, sigma, (L, q)), rng.normal(0, sigma, (L * (L - 1) // 2, q, q))


@pytest.mark.parametrize("L,q,randomize", [(9, 5, True), (14, 21, False), (5, 2, True)])
def test_all_sites_free_is_the_plain_restatement(L, q, randomize):
    h, Jp = random_model(L, q, 10 * L + q)
    n = 70
    chains = np.arange(3, 3 + n)
    X0 = np.random.default_rng(q).integers(0, q, size=(n, L), dtype=np.uint8)
    start = random_start(77, chains, L, q) if randomize else X0
    want, m0 = gibbs_ref(h, Jp, 0.8, 77, chains, 2, 4, start)
    got, m1 = cond_gibbs_ref(h, Jp, 0.8, 77, chains, 2, 4, X0, np.arange(L), randomize)
    assert min(m0, m1) > 1e-9                      # far above the two orders' difference: both pick the same state
    assert np.array_equal(got, want)


@pytest.mark.parametrize("free", [[0], [11], [0, 11], [3, 4, 5, 8, 9], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], []])
def test_masked_restatement_keeps_the_clamped_sites_and_agrees_with_the_full_sum(free):
    L, q = 12, 5
    h, Jp = random_model(L, q, 5)
    n = 50
    chains = np.arange(n)
    X0 = np.random.default_rng(1).integers(0, q, size=(n, L), dtype=np.uint8)
    free = np.array(free, dtype=np.int64)
    for randomize in (True, False):
        got, margin = cond_gibbs_ref(h, Jp, 1.0, 9, chains, 0, 3, X0, free, randomize)
        clamped = np.setdiff1d(np.arange(L), free)
        assert np.array_equal(got[:, clamped], X0[:, clamped])
        assert margin > 1e-9
        assert np.array_equal(got, masked_plain_ref(h, Jp, 1.0, 9, chains, 0, 3, X0, free, randomize))
    two, _ = cond_gibbs_ref(h, Jp, 1.0, 9, chains, 0, 2, X0, free, True)
    five, _ = cond_gibbs_ref(h, Jp, 1.0, 9, chains, 0, 5, X0, free, True)
    assert np.array_equal(cond_gibbs_ref(h, Jp, 1.0, 9, chains, 2, 3, two, free, False)[0], five)


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep," in header
    assert "const int32_t* free_sites, int num_free, const uint8_t* initial" in header
    assert '"cond_fields"' in header and '"sample_cond"' in header and "DESIGN.md section 23" in header
    assert "## 23." in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert hasattr(_lib.Context, "plm_sample_conditional") and hasattr(_lib.Context, "mf_sample_conditional")


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    X = np.zeros((2, 4), dtype=np.uint8)
    out = np.zeros((2, 4), dtype=np.uint8)
    sites = np.array([1, 2], dtype=np.int32)
    for name in ENTRIES:
        assert getattr(lib, name)(None, 2, 1, 0, 0, 0, 1.0, sites.ctypes.data, 2, X.ctypes.data, 1, out.ctypes.data) == _lib.DCA_ERR_ARG


# ---------------------------------------------------------------- Python argument checks
class Boom(Exception):
    pass


class Quiet:
    def info(self, *a):
        pass

    error = info


class Model(_potts.PottsModel):
    """PottsModel over a recorded _potts_call: L = 6 RNA sites"""
    _potts_exc = Boom
    _potts_table = 0
    _potts_logger = Quiet()

    def __init__(self, devices=None):
        self.calls, self.devices = [], devices

    def _potts_dims(self):
        return _lib.DCA_BIOMOLECULE_RNA, 6, 5

    def _potts_devices(self):
        return self.devices

    def _potts_call(self, name, *args, **kw):
        self.calls.append((name, args, kw))
        return np.asarray(args[0]).copy()


def test_free_and_fixed_sites_checks():
    m = Model()
    for kw in ({}, {"free_sites": [1], "fixed_sites": [2]}):
        with pytest.raises(Boom, match="exactly one"):
            m.sample_sequences_conditional("ACGUAC", **kw)
    with pytest.raises(Boom, match="twice"):
        m.sample_sequences_conditional("ACGUAC", free_sites=[1, 3, 1])
    with pytest.raises(Boom, match="twice"):
        m.sample_sequences_conditional("ACGUAC", fixed_sites=(2, 2))
    for bad in ([6], [-1, 2], [0, 99]):
        with pytest.raises(Boom, match="0 .. 5"):
            m.sample_sequences_conditional("ACGUAC", free_sites=bad)
    with pytest.raises(Boom, match="integers"):
        m.sample_sequences_conditional("ACGUAC", free_sites=[1.5])
    with pytest.raises(Boom, match="integers"):
        m.sample_sequences_conditional("ACGUAC", free_sites=3)
    with pytest.raises(Boom):
        m.sample_sequences_conditional("ACGUAC", free_sites=[1], temperature=0.0)
    with pytest.raises(Boom, match="template"):
        m.sample_sequences_conditional(None, free_sites=[1])
    assert m.calls == []                                        # every rejection came before the device call
    with pytest.raises(Boom, match="one GPU"):
        Model(devices=[0, 1]).sample_sequences_conditional("ACGUAC", free_sites=[1])


def test_sites_are_sorted_and_fixed_sites_name_the_complement():
    m = Model()
    out = m.sample_sequences_conditional("ACGUAC", free_sites=(4, 0, 2), num_sweeps=7, seed=3, temperature=2.0, randomize=False)
    assert out == ["ACGUAC"]
    name, args, kw = m.calls[-1]
    assert name == "sample_conditional" and args[0].tolist() == [[0, 1, 2, 3, 0, 1]]
    assert args[1].dtype == np.int32 and args[1].tolist() == [0, 2, 4] and args[2] == 7
    assert kw == {"seed": 3, "beta": 0.5, "random_start": False}
    m.sample_sequences_conditional("ACGUAC", fixed_sites=iter([5, 1]))
    assert m.calls[-1][1][1].tolist() == [0, 2, 3, 4] and m.calls[-1][2]["random_start"] is True
    m.sample_sequences_conditional("ACGUAC", fixed_sites=[])
    assert m.calls[-1][1][1].tolist() == [0, 1, 2, 3, 4, 5]
    m.sample_sequences_conditional("ACGUAC", free_sites=np.array([], dtype=np.int64))
    assert m.calls[-1][1][1].size == 0
    codes = m.sample_sequences_conditional("ACGUAC", free_sites=[1], return_codes=True)
    assert codes.dtype == np.uint8 and codes.shape == (1, 6)


def test_template_forms_and_counts(tmp_path):
    m = Model()
    assert len(m.sample_sequences_conditional("ACGUAC", free_sites=[1], num_sequences=4)) == 4        # one record is replicated
    assert m.calls[-1][1][0].tolist() == [[0, 1, 2, 3, 0, 1]] * 4
    assert m.sample_sequences_conditional(["ACGUAC", "UUUUUU", "------"], free_sites=[1]) == ["ACGUAC", "UUUUUU", "------"]
    with pytest.raises(Boom, match="holds 3 records"):
        m.sample_sequences_conditional(["ACGUAC", "UUUUUU", "------"], free_sites=[1], num_sequences=2)
    with pytest.raises(Boom, match="record 2"):
        m.sample_sequences_conditional(["ACGUAC", "UUUU"], free_sites=[1])
    with pytest.raises(Boom, match=">= 0"):
        m.sample_sequences_conditional("ACGUAC", free_sites=[1], num_sequences=-1)
    two = tmp_path / "two.fa"
    two.write_text(">a\nCCGGAA\n>b\nAAAAAA\n")
    assert m.sample_sequences_conditional(str(two), fixed_sites=[0]) == ["CCGGAA", "AAAAAA"]
    with pytest.raises(Boom, match="holds 2 records"):
        m.sample_sequences_conditional(str(two), fixed_sites=[0], num_sequences=5)
    one = tmp_path / "one.fa"
    one.write_text(">a\nCCGGAA\n")
    assert m.sample_sequences_conditional(str(one), fixed_sites=[0], num_sequences=3) == ["CCGGAA"] * 3


def test_context_binding_checks_the_shape():
    class Ctx(_lib.Context):
        def __init__(self):                                     # no device: only the host-side checks are reached
            self._l, self._h, self.L = _lib.lib(), None, 4
    with pytest.raises(ValueError, match="uint8"):
        Ctx().plm_sample_conditional(np.zeros((2, 5), dtype=np.uint8), [0], 1)
    with pytest.raises(ValueError, match="uint8"):
        Ctx().mf_sample_conditional(np.zeros(4, dtype=np.uint8), [0], 1)


# ---------------------------------------------------------------- the range parser
def test_site_range_parser():
    assert _potts.parse_site_ranges("3,1-2", Boom) == [2, 0, 1]
    assert _potts.parse_site_ranges(" 10-12 , 45 ", Boom) == [9, 10, 11, 44]
    assert _potts.parse_site_ranges("7", Boom) == [6]
    assert _potts.conditional_sites(_potts.parse_site_ranges("3,1-2", Boom), None, 5, Boom).tolist() == [0, 1, 2]
    for bad in ("", "5-4", "0", "0-3", "1,,2", "a", "1-b", "-3", "1-2-3", "2.5"):
        with pytest.raises(Boom):
            _potts.parse_site_ranges(bad, Boom)
    with pytest.raises(Boom, match="twice"):
        _potts.conditional_sites(_potts.parse_site_ranges("1-3,2", Boom), None, 5, Boom)


# ---------------------------------------------------------------- command lines
@pytest.mark.parametrize("main,run", [(plmdca_main, "run_plm_dca"), (mfdca_main, "run_meanfield_dca")])
def test_sample_conditional_arguments(monkeypatch, main, run):
    assert "sample_conditional" in _potts.POTTS_SUBCOMMANDS
    seen = {}
    monkeypatch.setattr(main, "execute_from_command_line", lambda *a, **kw: seen.update(kw) or "done")
    assert getattr(main, run)(["sample_conditional", "rna", "x.fa", "--template_file", "t.fa", "--free_sites", "10-30,45",
                               "--num_sequences", "7", "--num_sweeps", "30", "--seed", "11", "--temperature", "0.5",
                               "--keep_template_start"]) == "done"
    assert seen["the_command"] == "sample_conditional"
    assert seen["conditional"] == {"template_file": "t.fa", "free_sites": "10-30,45", "fixed_sites": None, "num_sequences": 7,
                                   "num_sweeps": 30, "seed": 11, "temperature": 0.5, "keep_template_start": True}
    getattr(main, run)(["sample_conditional", "rna", "x.fa", "--template_file", "t.fa", "--fixed_sites", "1-3"])
    assert seen["conditional"] == {"template_file": "t.fa", "free_sites": None, "fixed_sites": "1-3", "num_sequences": None,
                                   "num_sweeps": 1000, "seed": 0, "temperature": 1.0, "keep_template_start": False}
    for argv in (["--free_sites", "1"], ["--template_file", "t.fa"],
                 ["--template_file", "t.fa", "--free_sites", "1", "--fixed_sites", "2"]):
        with pytest.raises(SystemExit):
            getattr(main, run)(["sample_conditional", "rna", "x.fa"] + argv)
    with pytest.raises(SystemExit):                            # the plain sampler's sub-command does not take the new options
        getattr(main, run)(["sample_sequences", "rna", "x.fa", "--num_sequences", "2", "--free_sites", "1"])


class StandIn:
    """The calls run_subcommand makes for sample_conditional, recorded"""
    sequences_len = 10

    def __init__(self):
        self.calls = []

    def sample_sequences_conditional(self, template, **kw):
        self.calls.append(("sample", template, kw))
        return np.array([[0, 1, 2, 3, 4, 0, 1, 2, 3, 4], [4, 4, 4, 4, 4, 0, 0, 0, 0, 0]], dtype=np.uint8)

    def compute_sequence_energies(self, seqs):
        self.calls.append(("energies", list(seqs)))
        return np.array([-1.25, 1.0 / 3.0])


def test_subcommand_file(tmp_path):
    inst = StandIn()
    out = str(tmp_path / "out")
    opts = {"template_file": "t.fa", "free_sites": "8-9,2", "fixed_sites": None, "num_sequences": None, "num_sweeps": 12, "seed": None,
            "temperature": None, "keep_template_start": True}
    path = _potts.run_subcommand(inst, "sample_conditional", "MFDCA", TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA, 1,
                                 PlmDCAException, conditional=opts)
    assert os.path.basename(path) == "MFDCA_conditional_samples_toy_rna.fa"
    assert inst.calls[0] == ("sample", "t.fa", {"num_sequences": None, "num_sweeps": 12, "seed": 0, "temperature": 1.0,
                                                "randomize": False, "return_codes": True, "free_sites": [7, 8, 1]})
    assert inst.calls[1] == ("energies", ["ACGU-ACGU-", "-----AAAAA"])
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# Conditional Gibbs samples") and "3 free sites of 10" in lines[0]
    assert lines[1] == "# Free sites (1-based): 2,8,9"
    assert lines[2:] == [">sample_1 energy=-1.25", "ACGU-ACGU-", ">sample_2 energy=%.17g" % (1.0 / 3.0), "-----AAAAA"]
    assert fasta_reader.get_alignment_from_fasta_file(path) == ["ACGU-ACGU-", "-----AAAAA"]
    opts.update(free_sites=None, fixed_sites="1-8", keep_template_start=False)
    _potts.run_subcommand(inst, "sample_conditional", "MFDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 1, PlmDCAException,
                          conditional=opts)
    assert inst.calls[2][2]["fixed_sites"] == list(range(8)) and inst.calls[2][2]["randomize"] is True
    assert open(path).read().splitlines()[1] == "# Free sites (1-based): 9,10"
    for bad in ({"template_file": None}, {"free_sites": "1", "fixed_sites": "2"}, {"free_sites": None, "fixed_sites": None},
                {"fixed_sites": "11"}, {"fixed_sites": "0"}):
        with pytest.raises(PlmDCAException):
            _potts.run_subcommand(inst, "sample_conditional", "MFDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 1,
                                  PlmDCAException, conditional=dict(opts, **bad))
