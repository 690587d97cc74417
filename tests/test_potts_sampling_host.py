"""Host side of the Gibbs sampler: the Philox4x32-10 generator (dca_philox4x32_10) against the Random123 known-answer
vectors and a numpy restatement, the sample_sequences options of both command lines, the starting sequences and the FASTA
writer.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.dca_utilities import dca_utilities  # noqa: E402
from pydca_amd.fasta_reader import fasta_reader  # noqa: E402

M32 = 0xffffffff
# Random123 kat_vectors, philox4x32 with 10 rounds
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32,) * 4, (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox_np(ctr, key):
    """Philox4x32-10 on arrays of counters: ctr uint64[..., 4] (32-bit values), key (k0, k1) -> uint64[..., 4]."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., w] & M32 for w in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32), (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(M32), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(M32)]
    return np.stack(c, axis=-1)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert _lib.philox4x32_10(ctr, key).tolist() == list(want)
    assert philox_np(np.array(ctr, dtype=np.uint64), key).tolist() == list(want)


def test_philox_matches_restatement_on_many_counters():
    rng = np.random.default_rng(3)
    ctrs = rng.integers(0, 2 ** 32, size=(200, 4), dtype=np.uint64)
    key = (0x12345678, 0x9abcdef0)
    ref = philox_np(ctrs, key)
    got = np.array([_lib.philox4x32_10(c, key) for c in ctrs], dtype=np.uint64)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------- starting sequences
def test_initial_codes_forms(tmp_path):
    bio = _lib.DCA_BIOMOLECULE_RNA
    assert _potts.initial_codes(None, 3, bio, 4, 0, ValueError) is None
    X = _potts.initial_codes("ACGU", 3, bio, 4, 0, ValueError)                # one string: every chain starts from it
    assert X.shape == (3, 4) and X.tolist() == [[0, 1, 2, 3]] * 3
    X = _potts.initial_codes(["ACGU", "UUUU", "-A-A"], 3, bio, 4, 1, ValueError)
    assert X.tolist() == [[0, 1, 2, 3], [3, 3, 3, 3], [4, 0, 4, 0]]
    one = tmp_path / "one.fa"
    one.write_text(">a\nCCGG\n")
    assert _potts.initial_codes(str(one), 2, bio, 4, 0, ValueError).tolist() == [[1, 1, 2, 2]] * 2
    two = tmp_path / "two.fa"
    two.write_text(">a\nCCGG\n>b\nAAAA\n")
    assert _potts.initial_codes(str(two), 2, bio, 4, 0, ValueError).tolist() == [[1, 1, 2, 2], [0, 0, 0, 0]]


def test_initial_codes_rejections(tmp_path):
    class Boom(Exception):
        pass
    bio = _lib.DCA_BIOMOLECULE_RNA
    with pytest.raises(Boom, match="holds 2 records"):
        _potts.initial_codes(["ACGU", "ACGU"], 3, bio, 4, 0, Boom)
    f = tmp_path / "three.fa"
    f.write_text(">a\nACGU\n>b\nACGU\n>c\nACGU\n")
    with pytest.raises(Boom, match="holds 3 records"):
        _potts.initial_codes(str(f), 2, bio, 4, 0, Boom)
    with pytest.raises(Boom, match="record 2"):
        _potts.initial_codes(["ACGU", "AC7U", "ACGU"], 3, bio, 4, 0, Boom)
    with pytest.raises(Boom, match="record 3"):
        _potts.initial_codes(["ACGU", "ACGU", "ACG"], 3, bio, 4, 1, Boom)


@pytest.mark.parametrize("t", [0.0, -1.0, float("inf"), float("nan")])
def test_temperature_rejections(t):
    with pytest.raises(ValueError):
        _potts.sampling_beta(t, ValueError)
    assert _potts.sampling_beta(0.5, ValueError) == 2.0


@pytest.mark.parametrize("bio,table", [(_lib.DCA_BIOMOLECULE_PROTEIN, 0), (_lib.DCA_BIOMOLECULE_PROTEIN, 1),
                                       (_lib.DCA_BIOMOLECULE_RNA, 0), (_lib.DCA_BIOMOLECULE_RNA, 1)])
def test_state_letters_encode_back(bio, table):
    """The letters the samplers write encode back to the same codes under both readers' tables."""
    letters = _potts.state_letters(bio)
    q = len(letters)
    X = np.arange(q, dtype=np.uint8)[None, :]
    assert np.array_equal(_lib.encode_sequences(["".join(letters)], bio, q, table), X)


# ---------------------------------------------------------------- command lines
@pytest.mark.parametrize("main,run", [(plmdca_main, "run_plm_dca"), (mfdca_main, "run_meanfield_dca")])
def test_sample_sequences_arguments(monkeypatch, main, run):
    seen = {}
    monkeypatch.setattr(main, "execute_from_command_line", lambda *a, **kw: seen.update(kw) or "done")
    assert getattr(main, run)(["sample_sequences", "rna", "x.fa", "--num_sequences", "7", "--num_sweeps", "30", "--seed", "11",
                               "--temperature", "0.5", "--initial_file", "s.fa"]) == "done"
    assert seen["the_command"] == "sample_sequences"
    assert seen["sampling"] == {"num_sequences": 7, "num_sweeps": 30, "seed": 11, "temperature": 0.5, "initial_file": "s.fa"}
    getattr(main, run)(["sample_sequences", "rna", "x.fa", "--num_sequences", "2"])
    assert seen["sampling"] == {"num_sequences": 2, "num_sweeps": 1000, "seed": 0, "temperature": 1.0, "initial_file": None}
    with pytest.raises(SystemExit):                            # --num_sequences is required
        getattr(main, run)(["sample_sequences", "rna", "x.fa"])


def test_sampled_sequences_writer(tmp_path):
    path = str(tmp_path / "PLMDCA_samples_x.fa")
    seqs = ["ACGU-", "UUUUU", "A-C-G"]
    e = np.array([-1.25, 1.0 / 3.0, 12345.678901234567e-7])
    dca_utilities.write_sampled_sequences(path, seqs, e)
    lines = open(path).read().splitlines()
    assert lines[0] == ">sample_1 energy=-1.25"
    assert fasta_reader.get_alignment_from_fasta_file(path) == seqs
    back = np.array([float(ln.split("energy=")[1]) for ln in lines if ln.startswith(">")])
    assert back.tobytes() == e.tobytes()                       # %.17g round-trips bitwise
