"""Profile alignment on the device (align.hip): dca_profile_align and dca_sw_scores_device against the plain
restatement of the contract (tests/profile_align_reference.py) and against the host aligner.  Scores and residue_at are integers:
every comparison is for equality."""
import os

import numpy as np
import pytest

import profile_align_reference as R
from conftest import data_file
from pydca_amd import _lib, profile_alignment as PA
from pydca_amd.sequence_backmapper import scoring_matrix as sm

pytestmark = pytest.mark.gpu

MIXED = [0, 1, 2, 63, 64, 65, 200, 7, 31, 16, 33]        # lengths that meet in one wave
MODES = [R.LOCAL, R.GLOCAL]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, _lib.DCA_F32)
    yield c
    c.close()


def tables(rng, Lp, A, hi=9):
    return (rng.integers(-hi, hi + 1, size=(Lp, A)).astype(np.int32), -rng.integers(0, hi + 1, size=Lp).astype(np.int32),
            -rng.integers(0, hi + 1, size=Lp).astype(np.int32), -int(rng.integers(0, hi + 1)), -int(rng.integers(0, hi + 1)))


def queries(rng, A, lengths):
    return [rng.integers(0, A, size=int(n)).astype(np.uint8) for n in lengths]


def check(ctx, t, mode, seqs, want=None):
    """traceback run and score-only run == the reference; the invariants of residue_at -> the reference's (scores, residue_at)"""
    want = R.align_batch(*t, mode, seqs) if want is None else want
    score, res = ctx.profile_align(*t, mode, seqs)
    Lp = np.asarray(t[0]).shape[0]
    assert res.shape == (len(seqs), Lp) and res.dtype == np.int32
    bad = np.nonzero(score != want[0])[0]
    assert bad.size == 0, ("score", bad[:5], score[bad[:5]], want[0][bad[:5]])
    bad = np.nonzero((res != want[1]).any(axis=1))[0]
    assert bad.size == 0, ("residue_at", bad[:5], [len(seqs[k]) for k in bad[:5]])
    only, none = ctx.profile_align(*t, mode, seqs, traceback=False)
    assert none is None and np.array_equal(only, want[0])
    for k, s in enumerate(seqs):
        hit = res[k][res[k] >= 0]
        assert np.all(np.diff(hit) > 0) and (hit.size == 0 or hit[-1] < len(s))        # strictly increasing, inside the query
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Lp", [1, 2, 15, 16, 17, 33, 63, 64, 65, 97])       # T - 1, T, T + 1, 2T + 1 of both strip widths (16 below 64 columns, 32 from there)
def test_profile_lengths(ctx, Lp, mode):
    rng = np.random.default_rng(100 * Lp + mode)
    t = tables(rng, Lp, 21)
    check(ctx, t, mode, queries(rng, 21, (MIXED * 12)[:130]))


@pytest.mark.parametrize("mode", MODES)
def test_batch_sizes(ctx, mode):
    rng = np.random.default_rng(7 + mode)
    t = tables(rng, 33, 5, hi=5)
    seqs = queries(rng, 5, (MIXED * 12)[:130])
    want = R.align_batch(*t, mode, seqs)
    for n in (1, 63, 64, 65, 130):
        check(ctx, t, mode, seqs[-n:], (want[0][-n:], want[1][-n:]))
    score, res = ctx.profile_align(*t, mode, [])
    assert score.shape == (0,) and res.shape == (0, 33)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("A", [2, 5, 21, 27, 32])
def test_alphabets(ctx, A, mode):
    rng = np.random.default_rng(31 * A + mode)
    check(ctx, tables(rng, 70, A), mode, queries(rng, A, MIXED * 6))


@pytest.mark.parametrize("mode", MODES)
def test_tables_where_every_tie_rule_fires(ctx, mode):
    rng = np.random.default_rng(3 + mode)
    Lp, A = 37, 5
    seqs = queries(rng, A, [0, 1, 2, 5, 17, 36, 37, 38, 64, 90] * 7)
    zeros = np.zeros(Lp, dtype=np.int32)
    rnd = tables(rng, Lp, A, hi=3)
    check(ctx, (rnd[0], zeros, zeros, 0, 0), mode, seqs)                                   # all-zero penalties
    for c in (1, 0, -1):
        const = np.full((Lp, A), c, dtype=np.int32)
        check(ctx, (const, zeros, zeros, 0, 0), mode, seqs)                                # constant scores, free gaps
        check(ctx, (const, zeros - 1, zeros, -1, 0), mode, seqs)
        check(ctx, (const, zeros - 1, zeros - 1, -1, -1), mode, seqs)
    homo = [np.zeros(n, dtype=np.uint8) for n in (1, 3, 36, 37, 38, 80)]                   # homopolymers against a two-valued table
    two = np.where(np.arange(A)[None, :] == 0, 2, -1).astype(np.int32).repeat(Lp, axis=0)
    check(ctx, (two, zeros - 2, zeros - 1, -2, -1), mode, homo * 11)


@pytest.mark.parametrize("mode", MODES)
def test_profile_longer_than_every_query_and_the_reverse(ctx, mode):
    rng = np.random.default_rng(11 + mode)
    check(ctx, tables(rng, 150, 21), mode, queries(rng, 21, [0, 1, 2, 3, 4, 5] * 12))
    check(ctx, tables(rng, 3, 21), mode, queries(rng, 21, [3, 4, 64, 129, 200, 300] * 11))


@pytest.mark.parametrize("mode", MODES)
def test_values_at_the_argument_bound(ctx, mode):
    """(max|match| + max|penalty|) * (Lp + 32767) < 2^28 at Lp = 20: 8187 * 32787 = 268427169 passes, 8188 does not"""
    rng = np.random.default_rng(13 + mode)
    Lp, A = 20, 5
    match = rng.integers(-4000, 4001, size=(Lp, A)).astype(np.int32)
    match[0, 0], match[1, 1] = 4000, -4000
    do, de = -rng.integers(0, 4188, size=Lp).astype(np.int32), -rng.integers(0, 4188, size=Lp).astype(np.int32)
    do[3] = -4187
    check(ctx, (match, do, de, -4187, -1), mode, queries(rng, A, [0, 1, 19, 20, 21, 64, 150] * 10))
    # the sums the bound allows: the largest query against constant extremes (the score is 20 * 4000 or the boundary's deletions)
    long_ = [np.zeros(32767, dtype=np.uint8)]
    score, _ = ctx.profile_align(np.full((Lp, A), 4000, dtype=np.int32), np.full(Lp, -4187), np.full(Lp, -4187), -4187, -4187, mode,
                                 long_, traceback=False)
    assert score[0] == 20 * 4000
    score, _ = ctx.profile_align(np.full((Lp, A), -4000, dtype=np.int32), np.full(Lp, -4187), np.full(Lp, -4187), -4187, -4187, mode,
                                 long_, traceback=False)
    assert score[0] == (0 if mode == R.LOCAL else -20 * 4000)      # glocal: twenty mismatches (-80000) beat twenty deletions (-83740)


@pytest.mark.parametrize("mode", MODES)
def test_passes_give_the_same_bits(ctx, mode, monkeypatch):
    rng = np.random.default_rng(17 + mode)
    t = tables(rng, 70, 21)
    seqs = queries(rng, 21, (MIXED * 12)[:130])
    want = check(ctx, t, mode, seqs)
    for per_pass in ("1", "64", "100"):
        monkeypatch.setenv("DCA_ALIGN_PASS", per_pass)
        check(ctx, t, mode, seqs, want)
    monkeypatch.delenv("DCA_ALIGN_PASS")
    check(ctx, t, mode, seqs, want)                                                        # and under a second call


@pytest.mark.parametrize("mode", MODES)
def test_match_table_staged_strip_by_strip(ctx, mode):
    """3000 x 32 x 4 bytes is more than the LDS budget of a whole table (align_plan.h): the table is staged per strip"""
    rng = np.random.default_rng(19 + mode)
    check(ctx, tables(rng, 3000, 32, hi=5), mode, queries(rng, 32, [0, 1, 2, 3, 5, 8, 8] * 10))


def fixture_pair(msa, ref):
    rows = [s.upper().replace("-", "").replace(".", "") for s in PA.fasta_records(data_file(msa))[1]]
    return PA.fasta_records(data_file(ref))[1][0].strip().upper(), rows


@pytest.mark.parametrize("msa,ref,bio", [("PF02826.faa", "ref_seq_PF02826.faa", "PROTEIN"),
                                         ("MSA_RF00059_trimmed_gap_treshold_50.fa", "ref_seq_RF00059.faa", "RNA")])
def test_device_smith_waterman_equals_the_host_aligner(ctx, msa, ref, bio):
    refseq, rows = fixture_pair(msa, ref)
    sub, (go, ge) = sm.MATRICES[bio], sm.GAP_PENALTIES[bio]
    host = _lib.sw_scores(refseq, rows, sub, go, ge)
    assert np.array_equal(ctx.sw_scores(refseq, rows, sub, go, ge), host)
    score, res = ctx.profile_align(*R.sw_profile(refseq, sub, go, ge), R.LOCAL, [R.sw_codes(s) for s in rows])
    assert np.array_equal(score, host)
    for k, s in enumerate(rows):
        a, b, sc, sa, sb = _lib.sw_align(refseq, s, sub, go, ge)
        assert list(res[k]) == R.residue_at_from_pair(len(refseq), a, b, sa, sb), k
    odd = ["", "ACGU", "acgu", "AC-GU", "XXXX", "AC?GU*"]                                   # characters outside the 26 letters
    assert np.array_equal(ctx.sw_scores(refseq, odd, sub, go, ge), _lib.sw_scores(refseq, odd, sub, go, ge))
    assert np.array_equal(ctx.sw_scores("AC?gU", odd, sub, go, ge), _lib.sw_scores("AC?gU", odd, sub, go, ge))


@pytest.mark.parametrize("msa,ref,bio", [("MSA_RF00059_trimmed_gap_treshold_50.fa", "ref_seq_RF00059_test2.faa", "rna"),
                                         ("PF02826.faa", "ref_seq_PF02826.faa", "protein")])
def test_backmapper_gives_the_same_mapping_on_the_device(msa, ref, bio, monkeypatch):
    from pydca_amd.sequence_backmapper.sequence_backmapper import SequenceBackmapper
    calls = []
    real = _lib.Context.sw_scores
    monkeypatch.setattr(_lib.Context, "sw_scores", lambda self, *a: calls.append(1) or real(self, *a))

    def run():
        bm = SequenceBackmapper(msa_file=data_file(msa), refseq_file=data_file(ref), biomolecule=bio)
        return bm.find_matching_seqs_from_alignment(), bm.map_to_reference_sequence()
    monkeypatch.setenv("DCA_SW_DEVICE", "0")
    host = run()
    assert not calls
    monkeypatch.delenv("DCA_SW_DEVICE")
    assert run() == host
    assert calls or host[0][0].replace("-", "") == PA.fasta_records(data_file(ref))[1][0].strip().upper()    # (no search: the first row is it)


def test_end_to_end_on_the_toy_protein_alignment():
    """Rows stripped of their gaps and aligned back (glocal): where the REFERENCE alignment reproduces the row, the energy of the
    device-aligned string has the bits of the row's energy."""
    from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
    path = data_file("toy_protein.fa")
    rows = [s.upper() for s in PA.fasta_records(path)[1]]
    raw = [s.replace("-", "") for s in rows]
    inst = MeanFieldDCA(path, "protein")
    out = inst.align_sequences(raw)
    c = inst._compare_context()
    P = PA.build_profile(c.msa(), c.weights(), 21)
    table = PA.letter_codes(_lib.PROTEIN, 21)
    codes = [table[np.frombuffer(s.encode(), dtype=np.uint8)] for s in raw]
    want = R.align_batch(P["match"], P["del_open"], P["del_extend"], P["ins_open"], P["ins_extend"], R.GLOCAL, codes)
    assert np.array_equal(out["scores"], want[0]) and np.array_equal(out["residue_at"], want[1])
    assert (out["residue_at"] >= 0).sum(axis=1).tolist() == [len(s) - n for s, n in zip(raw, out["num_inserted"])]
    ref_strings = PA.aligned_strings(raw, want[1])
    same = [k for k in range(len(rows)) if ref_strings[k] == rows[k]]
    print("rows the reference alignment reproduces: %d of %d" % (len(same), len(rows)))
    assert same
    E_rows = inst.compute_sequence_energies([rows[k] for k in same])
    E_aligned = inst.compute_sequence_energies([out["aligned"][k] for k in same])
    assert E_aligned.tobytes() == E_rows.tobytes()
    a2m = inst.align_sequences(raw, format="a2m")["aligned"]
    assert [s.replace("-", "").upper() for s in a2m] == raw
    assert ["".join(ch for ch in s if not ch.islower()) for s in a2m] == out["aligned"]
    local = inst.align_sequences(raw, mode="local")
    assert np.all(local["scores"] >= 0) and len(local["aligned"][0]) == len(rows[0])
    with pytest.raises(Exception, match="align_sequences"):
        inst.align_sequences(raw, mode="global")
    with pytest.raises(Exception, match="align_sequences"):
        inst.align_sequences(raw, pseudocount=0.0)


@pytest.mark.parametrize("which", ["plmdca", "ardca"])
def test_mixin_on_the_other_two_classes(which):
    """PlmDCA and ArDCA fit on the de-duplicated alignment; ArDCA's context holds its columns in model order, the profile must not"""
    path = data_file("toy_protein.fa")
    rows = [s.upper() for s in PA.fasta_records(path)[1]]
    raw = [s.replace("-", "") for s in rows[:10]] + ["MKV", ""]
    if which == "plmdca":
        from pydca_amd.plmdca.plmdca import PlmDCA
        inst = PlmDCA(path, "protein", seqid=0.8, lambda_h=1.0, lambda_J=5.0, max_iterations=5)
    else:
        from pydca_amd.ardca.ardca import ArDCA
        inst = ArDCA(path, "protein")
    out = inst.align_sequences(raw)
    X, _raw = _lib.read_msa(path, _lib.PROTEIN, len(rows[0]))                              # file order of the columns
    P = PA.build_profile(X, inst._compare_context().weights(), 21)
    table = PA.letter_codes(_lib.PROTEIN, 21)
    codes = [table[np.frombuffer(s.encode(), dtype=np.uint8)] for s in raw]
    want = R.align_batch(P["match"], P["del_open"], P["del_extend"], P["ins_open"], P["ins_extend"], R.GLOCAL, codes)
    assert np.array_equal(out["scores"], want[0]) and np.array_equal(out["residue_at"], want[1])
    assert out["aligned"] == PA.aligned_strings(raw, want[1]) and out["aligned"][-1] == "-" * len(rows[0])
    again = inst.align_sequences(raw, pseudocount=0.5)                                     # other profile_args: another profile
    assert inst.align_sequences(raw)["scores"].tolist() == out["scores"].tolist() and len(again["aligned"]) == len(raw)


def test_profile_aligner_class_and_command_line(tmp_path):
    from pydca_amd import main
    path = data_file("toy_rna.fa")
    rows = [s.upper() for s in PA.fasta_records(path)[1]]
    raw = [s.replace("-", "") for s in rows][:12] + ["", "ACGUNNACGU"]
    with PA.ProfileAligner(path, "rna", seqid=0.8) as al:
        out = al.align(raw)
        P = al.profile
        codes = [al._table[np.frombuffer(s.encode(), dtype=np.uint8)] for s in raw]
        want = R.align_batch(P["match"], P["del_open"], P["del_extend"], P["ins_open"], P["ins_extend"], R.GLOCAL, codes)
        assert np.array_equal(out["scores"], want[0]) and np.array_equal(out["residue_at"], want[1])
        assert all(len(s) == len(rows[0]) for s in out["aligned"]) and out["aligned"][12] == "-" * len(rows[0])
    fa = tmp_path / "raw.fa"
    fa.write_text("".join(">r%d\n%s\n" % (k, s) for k, s in enumerate(raw)))
    files = main.run_pydca(["align_sequences", "rna", path, str(fa), "--output_dir", str(tmp_path / "out")])
    assert [os.path.basename(f) for f in files] == ["Aligned_raw.fa", "Aligned_raw_scores.txt"]
    assert PA.fasta_records(files[0]) == (["r%d" % k for k in range(len(raw))], out["aligned"])
    assert [int(ln.split("\t")[2]) for ln in open(files[1]).read().splitlines()[2:]] == out["scores"].tolist()


def test_errors(ctx):
    rng = np.random.default_rng(23)
    t = tables(rng, 20, 5)
    seqs = queries(rng, 5, [3, 4])

    def fails(tt, mode=R.GLOCAL, s=seqs, text=None):
        with pytest.raises(_lib.DcaBackendError, match=text) as e:
            ctx.profile_align(*tt, mode, s)
        assert e.value.code == _lib.DCA_ERR_ARG
    fails((np.zeros((8193, 2), dtype=np.int32), np.zeros(8193), np.zeros(8193), 0, 0), text="Lp")
    fails((np.zeros((0, 5), dtype=np.int32), np.zeros(0), np.zeros(0), 0, 0))
    fails((np.zeros((4, 1), dtype=np.int32), np.zeros(4), np.zeros(4), 0, 0), s=[np.zeros(2, dtype=np.uint8)], text="A 1")
    fails((np.zeros((4, 33), dtype=np.int32), np.zeros(4), np.zeros(4), 0, 0), text="A 33")
    fails(t, mode=2, text="mode")
    for k in (1, 2):
        pen = [t[1].copy(), t[2].copy()]
        pen[k - 1][7] = 1
        fails((t[0], pen[0], pen[1], t[3], t[4]), text="column 7")
    fails((t[0], t[1], t[2], 1, 0), text="ins_open")
    fails((t[0], t[1], t[2], 0, 1), text="ins_extend")
    at = (np.full((20, 5), 4000, dtype=np.int32), np.full(20, -4187), np.full(20, -4187), -4187, -4188)
    fails(at, text="2\\^28")                                                              # 8188 * 32787 >= 2^28
    ctx.profile_align(at[0], at[1], at[2], -4187, -4187, R.GLOCAL, seqs)                  # 8187 passes
    fails(t, s=[seqs[0], np.array([0, 5, 1], dtype=np.uint8)], text="record 1")           # a code >= A names its record
    fails(t, s=[np.zeros(32768, dtype=np.uint8)], text="record 0")
    sub = sm.MATRICES["RNA"]
    with pytest.raises(_lib.DcaBackendError):
        ctx.sw_scores("ACGU", ["ACGU"], sub, 1, 0)                                         # a positive gap penalty
    with pytest.raises(_lib.DcaBackendError):
        ctx.sw_scores("A" * 8193, ["ACGU"], sub, -8, 0)
    assert ctx.profile_align_last_scratch() >= 0
