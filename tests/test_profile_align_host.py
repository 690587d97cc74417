"""Profile alignment, the parts that need no GPU: the plain restatement of the contract
(tests/profile_align_reference.py) against the Smith-Waterman oracle and the library's host aligner, whose results the device
entries must reproduce; build_profile; the launch plan (pydca_amd/csrc/align_plan.h, compiled alone); argument validation of
the Python entry and the command line."""
import os
import subprocess

import numpy as np
import pytest

import profile_align_reference as R
from conftest import data_file
from pydca_amd import _lib, main, profile_alignment as PA
from pydca_amd.sequence_backmapper import scoring_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fasta_rows(name):
    return PA.fasta_records(data_file(name))[1]


def random_tables(rng, Lp, A, hi=9):
    return (rng.integers(-hi, hi + 1, size=(Lp, A)).astype(np.int32), -rng.integers(0, hi + 1, size=Lp).astype(np.int32),
            -rng.integers(0, hi + 1, size=Lp).astype(np.int32), -int(rng.integers(0, hi + 1)), -int(rng.integers(0, hi + 1)))


def test_reference_local_mode_is_the_smith_waterman_oracle():
    from oracle import sw
    rng = np.random.default_rng(5)
    for bio, alphabet in (("PROTEIN", "ARNDCQEGHILKMFPSTWYV"), ("RNA", "ACGU")):
        sub, (go, ge) = sm.MATRICES[bio], sm.GAP_PENALTIES[bio]
        score = lambda x, y: int(sub[ord(x) - 65, ord(y) - 65])
        for _ in range(6):
            ref = "".join(rng.choice(list(alphabet), int(rng.integers(1, 30))))
            s = "".join(rng.choice(list(alphabet), int(rng.integers(0, 30))))
            got = R.align_one(*R.sw_profile(ref, sub, go, ge), R.LOCAL, R.sw_codes(s))[0]
            assert got == sw.local_score(ref, s, score, go, ge)


def check_against_host_aligner(ref, rows, sub, go, ge, scalar=2):
    """scores and traceback of the reference (batched; the first `scalar` rows also cell by cell) == dca_sw_scores, dca_sw_align"""
    prof = R.sw_profile(ref, sub, go, ge)
    codes = [R.sw_codes(s) for s in rows]
    scores, res = R.align_batch(*prof, R.LOCAL, codes)
    assert list(scores) == list(_lib.sw_scores(ref, rows, sub, go, ge))
    for k, s in enumerate(rows):
        a, b, sc, sa, sb = _lib.sw_align(ref, s, sub, go, ge)
        assert sc == scores[k]
        assert list(res[k]) == R.residue_at_from_pair(len(ref), a, b, sa, sb), (k, s)
        if k < scalar:
            one = R.align_one(*prof, R.LOCAL, codes[k])
            assert one[0] == sc and one[1] == list(res[k]) and one[2] == (sa, sb)       # the starts: where the traceback stopped


@pytest.mark.parametrize("msa,ref,bio", [("PF02826.faa", "ref_seq_PF02826.faa", "PROTEIN"),
                                         ("MSA_RF00059_trimmed_gap_treshold_50.fa", "ref_seq_RF00059.faa", "RNA")])
def test_reference_equals_the_host_aligner_on_the_backmapping_fixtures(msa, ref, bio):
    rows = [s.upper().replace("-", "").replace(".", "") for s in fasta_rows(msa)]
    refseq = fasta_rows(ref)[0].strip().upper()
    pick = rows[:12] + rows[len(rows) // 2:len(rows) // 2 + 6]
    check_against_host_aligner(refseq, pick, sm.MATRICES[bio], *sm.GAP_PENALTIES[bio])


def test_reference_equals_the_host_aligner_where_every_tie_rule_fires():
    sub = sm.MATRICES["PROTEIN"]
    homo = ["AAAAAAA", "AAA", "A", "", "AAAAAAAAAAAA", "AAGAA", "GGGG"]
    check_against_host_aligner("AAAAAA", homo, sub, -10, -1, scalar=7)
    check_against_host_aligner("AAAAAA", homo, sub, 0, 0, scalar=7)              # zero gap penalties
    check_against_host_aligner("ACACAC", ["CACACA", "ACAC", "AACC", "CCAA", "AXC?A"], sub, 0, 0, scalar=5)
    check_against_host_aligner("ACGUACGU", ["ACGACGU", "ACGUUACGU", "UGCA"], sm.MATRICES["RNA"], -8, 0, scalar=3)
    const = np.full((26, 26), 1, dtype=np.int32)                                # constant scores
    check_against_host_aligner("AAAA", ["AAAAAA", "AA", "CCCCC"], const, -1, 0, scalar=3)


@pytest.mark.parametrize("mode", [R.LOCAL, R.GLOCAL])
def test_batched_reference_equals_the_cell_by_cell_one(mode):
    rng = np.random.default_rng(17 + mode)
    for Lp, A in ((1, 2), (3, 5), (7, 21), (12, 32)):
        t = random_tables(rng, Lp, A, hi=4)
        seqs = [rng.integers(0, A, size=int(n)).astype(np.uint8) for n in (0, 1, 2, 5, 9, 15)]
        scores, res = R.align_batch(*t, mode, seqs)
        for k, s in enumerate(seqs):
            one = R.align_one(*t, mode, s)
            assert one[0] == scores[k] and one[1] == list(res[k])
            hit = [r for r in one[1] if r >= 0]
            assert hit == sorted(set(hit))                                   # strictly increasing


def test_glocal_boundary_and_empty_query():
    match = np.array([[2, -1], [2, -1], [2, -1]], dtype=np.int32)
    do, de = np.array([-3, -4, -5], dtype=np.int32), np.array([-9, -1, -2], dtype=np.int32)
    score, res, _s, end = R.align_one(match, do, de, -2, -1, R.GLOCAL, [])
    assert score == -3 - 1 - 2 and res == [-1, -1, -1] and end == (3, 0)      # del_open[1] + del_extend[2] + del_extend[3]
    score, res, _s, end = R.align_one(match, do, de, -2, -1, R.GLOCAL, [1, 0, 0, 0, 1])
    assert score == 6 and res == [1, 2, 3] and end == (3, 4)                  # overhangs are free


# ---------------------------------------------------------------- build_profile
def toy(name, q):
    bio = _lib.PROTEIN if q == 21 else _lib.RNA
    rows = [s.upper() for s in fasta_rows(name)]
    X = _lib.encode_sequences(rows, bio, len(rows[0]), 1)
    w = 1.0 / (1.0 + np.arange(X.shape[0]) % 3)                                # any positive weights serve
    return X, w


@pytest.mark.parametrize("name,q", [("toy_protein.fa", 21), ("toy_rna.fa", 5)])
def test_build_profile(name, q):
    X, w = toy(name, q)
    X = X.copy()
    X[:, 2] = q - 1                                                            # an all-gap column
    P = PA.build_profile(X, w, q)
    L = X.shape[1]
    assert P["match"].shape == (L, q) and P["match"].dtype == np.int32
    assert P["del_open"].shape == (L,) and P["del_extend"].shape == (L,)
    assert (P["del_open"] <= 0).all() and (P["del_extend"] <= 0).all() and P["ins_open"] <= 0 and P["ins_extend"] <= 0
    assert P["ins_open"] == -192 and P["ins_extend"] == -32                    # rint(32 * -6), rint(32 * -1)
    assert not P["match"][2].any()                                             # the all-gap column scores nothing
    assert P["del_open"][2] == 0                                               # ... and costs nothing to skip: log2(1)
    assert not P["match"][:, q - 1].any()                                      # the unknown residue
    assert P["match"].any()
    assert P["del_extend"][0] == P["del_open"][0]
    floor = int(np.rint(32 * np.log2(0.02)))
    assert P["del_open"].min() >= floor and P["del_extend"].min() >= floor
    perm = np.random.default_rng(3).permutation(X.shape[0])
    Q = PA.build_profile(X[perm], w[perm], q)
    for k in ("match", "del_open", "del_extend"):
        assert np.array_equal(P[k], Q[k]), k                                   # the same bits for any order of the rows
    # a conserved column scores its residue above the others, and the formula of the docstring at one entry
    wq = np.rint(w * 2.0 ** 30)
    col = int(np.argmax([(X[:, c] != q - 1).sum() for c in range(L)]))
    counts = np.array([wq[X[:, col] == a].sum() for a in range(q - 1)])
    assert counts.sum() > 0
    a = int(np.argmax(counts))
    res_cols = [c for c in range(L) if (X[:, c] != q - 1).any()]
    r = lambda c: np.array([wq[X[:, c] == b].sum() for b in range(q - 1)]) / sum(wq[X[:, c] == b].sum() for b in range(q - 1))
    bg = 0.8 * np.mean([r(c) for c in res_cols], axis=0) + 0.2 / (q - 1)
    want = np.rint(32 * np.log2((0.8 * r(col)[a] + 0.2 * bg[a]) / bg[a]))
    assert abs(int(P["match"][col, a]) - int(want)) <= 1                        # (summation order of the mean: at most one unit)


def test_build_profile_rejects_bad_arguments():
    X, w = toy("toy_rna.fa", 5)
    for kw in (dict(pseudocount=0.0), dict(pseudocount=1.5), dict(deletion_floor=0.0), dict(ins_open_bits=1.0), dict(scale=0)):
        with pytest.raises(ValueError):
            PA.build_profile(X, w, 5, **kw)
    with pytest.raises(ValueError):
        PA.build_profile(X, w[:-1], 5)
    with pytest.raises(ValueError):
        PA.build_profile(X, w, 4)                                              # a code >= q
    with pytest.raises(ValueError):
        PA.build_profile(X, -w, 5)


# ---------------------------------------------------------------- the launch plan, compiled alone
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("align_plan")), "align_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "align_plan_driver.cpp")])

    def run(groups):
        """groups: (Lp, A, traceback, maxLen, envPass) -> one dict per group"""
        out = []
        for ln in subprocess.check_output([exe] + [str(v) for g in groups for v in g]).decode().splitlines():
            tok = ln.split()
            out.append({k: int(v) for k, v in zip(tok[::2], tok[1::2])})
        return out
    return run


def test_launch_plan(plan):
    GiB, KiB = 1 << 30, 1 << 10
    cases = [(Lp, A, tr, ml, env) for Lp in (1, 2, 15, 16, 17, 63, 64, 65, 500, 511, 512, 513, 3000, 8191, 8192) for A in (2, 5, 21, 27, 32)
             for tr in (0, 1) for ml, env in ((0, -1), (1, -1), (500, -1), (32767, -1), (500, 1), (500, 100))]
    for c, p in zip(cases, plan(cases)):
        Lp, A, tr, ml, env = c
        assert p["T"] == (32 if Lp >= 64 else 16) and p["strips"] == -(-Lp // p["T"]) and p["LpPad"] == p["strips"] * p["T"]
        whole_bytes = A * (p["LpPad"] + 4) * 4
        assert p["whole"] == int(whole_bytes <= 64 * KiB), c
        assert p["ldsStride"] == (p["LpPad"] if p["whole"] else p["T"]) + 4 and p["ldsStride"] % 16 == 4
        assert p["ldsBytes"] == A * p["ldsStride"] * 4 <= 64 * KiB <= p["ldsMax"] == 160 * KiB
        assert p["bytesPerResidue"] == 8 + (p["LpPad"] // 2 if tr else 0)
        assert p["bytesPerQuery"] == p["bytesPerResidue"] * max(ml, 1)
        assert p["queriesPerPass"] >= 1 and p["passBytes"] <= GiB == p["scratchMax"], c
        if env > 0:
            assert p["queriesPerPass"] <= env
        else:
            assert p["queriesPerPass"] == min(GiB // p["bytesPerQuery"], 1 << 24)
    edge = plan([(512, 32, 1, 1, -1), (480, 32, 1, 1, -1), (3000, 32, 1, 8, -1), (8192, 2, 1, 32767, -1), (500, 27, 0, 500, -1),
                 (500, 21, 1, 500, -1)])
    assert [p["whole"] for p in edge] == [0, 1, 0, 0, 1, 1]           # 32 * 516 * 4 = 66048 > 65536 >= 32 * 484 * 4
    assert edge[3]["queriesPerPass"] == 7 and edge[3]["bytesPerQuery"] == 32767 * (8 + 4096)      # the largest single query: 128.3 MiB
    assert edge[4]["queriesPerPass"] == GiB // 4000 and edge[5]["bytesPerQuery"] == 500 * (8 + 256)


def test_launch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "align_plan_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "align_plan_driver.cpp")])
    args = [str(v) for g in ((1, 2, 0, 0, -1), (8192, 32, 1, 32767, 1), (8192, 32, 1, 32767, 1 << 40), (64, 21, 1, 0, 0)) for v in g]
    assert len(subprocess.check_output([exe] + args).decode().splitlines()) == 4


# ---------------------------------------------------------------- Python entry and command line, without a device
def test_raw_records_and_strings():
    assert PA.raw_records(["ac-g.u", "", "ACGU"]) == ["ACGU", "", "ACGU"]
    for bad in (["AC1"], ["AC G"], None, "no_such_file.fa"):
        with pytest.raises(ValueError):
            PA.raw_records(bad)
    with pytest.raises(ValueError):
        PA.raw_records(["A" * 32768])
    res = np.array([[1, -1, 3], [-1, -1, -1]], dtype=np.int32)
    assert PA.aligned_strings(["XACDEF", "GG"], res) == ["A-D", "---"]
    assert PA.aligned_strings(["XACDEF", "GG"], res, "a2m") == ["xA-cDef", "---gg"]
    for mode, fmt in (("global", "aligned"), ("glocal", "fasta")):
        with pytest.raises(ValueError):
            PA.check_mode_format(mode, fmt)
    table = PA.letter_codes(_lib.RNA, 5)
    assert sorted(table[[ord(c) for c in "ACGU"]]) == [0, 1, 2, 3] and table[ord("N")] == 4 and table[ord("-")] == 4


def test_fasta_records_of_any_length(tmp_path):
    path = tmp_path / "raw.fa"
    path.write_text(">one first\nACGU\nAC\n>two\n\n>three\nGG\n")
    assert PA.fasta_records(str(path)) == (["one", "two", "three"], ["ACGUAC", "", "GG"])
    assert PA.raw_records(str(path)) == ["ACGUAC", "", "GG"]


def test_command_line(tmp_path, monkeypatch):
    raw = tmp_path / "queries.fa"
    raw.write_text(">q1\nACGU\n>q2\nGGAC\n")
    seen = {}

    class Stub:
        def __init__(self, msa_file, biomolecule, seqid=0.8, device=0):
            seen.update(msa=msa_file, bio=biomolecule, seqid=seqid, device=device)

        def align(self, sequences, mode, format):
            seen.update(seqs=list(sequences), mode=mode, format=format)
            n = len(sequences)
            return dict(aligned=["AC-u"] * n, scores=np.arange(n, dtype=np.int32), residue_at=np.array([[0, 1, -1]] * n),
                        num_inserted=np.full(n, 2, dtype=np.int32))

    monkeypatch.chdir(tmp_path)
    files = PA.execute("msa.fa", "rna", str(raw), mode="local", a2m=True, seqid=0.7, device=0, aligner_class=Stub)
    assert [os.path.relpath(f, str(tmp_path)) for f in files] == [os.path.join("Aligned_queries", "Aligned_queries.fa"),
                                                                  os.path.join("Aligned_queries", "Aligned_queries_scores.txt")]
    assert seen == dict(msa="msa.fa", bio="rna", seqid=0.7, device=0, seqs=["ACGU", "GGAC"], mode="local", format="a2m")
    assert open(files[0]).read() == ">q1\nAC-u\n>q2\nAC-u\n"
    assert open(files[1]).read().splitlines()[2:] == ["0\tq1\t0\t2\t2", "1\tq2\t1\t2\t2"]
    with pytest.raises(SystemExit):
        main.run_pydca(["align_sequences", "rna", "msa.fa", str(raw), "--mode", "global"])
    with pytest.raises(SystemExit):
        main.run_pydca(["align_sequences", "rna", "msa.fa"])
    called = {}
    monkeypatch.setattr(PA, "execute", lambda *a, **k: called.update(a=a, k=k) or ["x"])
    assert main.run_pydca(["align_sequences", "rna", "msa.fa", str(raw), "--a2m", "--output_dir", "out"]) == ["x"]
    assert called["a"] == ("msa.fa", "rna", str(raw)) and called["k"] == dict(mode="glocal", a2m=True, seqid=0.8, device=0, output_dir="out")


def test_exports_and_mixin():
    for name in ("dca_profile_align", "dca_sw_scores_device", "dca_profile_align_last_scratch", "dca_get_msa"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    from pydca_amd.ardca.ardca import ArDCA
    from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
    from pydca_amd.plmdca.plmdca import PlmDCA
    for cls in (PlmDCA, MeanFieldDCA, ArDCA):
        assert issubclass(cls, PA.SequenceAlignment) and callable(cls.align_sequences)
