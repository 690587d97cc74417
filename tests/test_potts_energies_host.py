"""Host side of the Potts energy feature: the query encoder (dca_encode_sequences) and the two output writers.
No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts  # noqa: E402
from pydca_amd.dca_utilities import dca_utilities  # noqa: E402
from pydca_amd.fasta_reader import fasta_reader  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
FASTA = [("toy_rna.fa", "RNA"), ("toy_protein.fa", "PROTEIN"), ("MSA_RF00167.fa", "RNA"), ("PF02826.faa", "PROTEIN"),
         ("MSA_RF00059_trimmed_gap_treshold_50.fa", "RNA")]
# files with one sequence per line (what the plm reader reads)
ONE_LINE = [("toy_rna.fa", "RNA"), ("toy_protein.fa", "PROTEIN"), ("MSA_RF00167.fa", "RNA")]


def _bio(name):
    return _lib.DCA_BIOMOLECULE_PROTEIN if name == "PROTEIN" else _lib.DCA_BIOMOLECULE_RNA


def _mf_restatement(seqs, biomolecule):
    """The mf reader's table (fasta_reader.RES_TO_INT_ALL, unknown -> gap), 0-based, every record kept."""
    q = 21 if biomolecule == "PROTEIN" else 5
    table = np.full(256, q, dtype=np.int64)
    for ch, v in fasta_reader.RES_TO_INT_ALL[biomolecule].items():
        table[ord(ch)] = v
    return np.array([table[np.frombuffer(s.upper().encode("latin-1"), dtype=np.uint8)] - 1 for s in seqs], dtype=np.uint8)


def _first_occurrence(X):
    seen, keep = set(), []
    for k, row in enumerate(X):
        key = row.tobytes()
        if key not in seen:
            seen.add(key)
            keep.append(k)
    return X[keep]


@pytest.mark.parametrize("fname,bio", FASTA)
def test_encoder_mf_table_matches_reader(fname, bio):
    path = os.path.join(DATA, fname)
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    X = _lib.encode_sequences(seqs, _bio(bio), len(seqs[0]), 1)
    assert X.shape == (len(seqs), len(seqs[0]))                   # no de-duplication, input order
    assert np.array_equal(X, _mf_restatement(seqs, bio))
    int_form = np.array(fasta_reader.get_alignment_int_form(path, biomolecule=bio), dtype=np.int64) - 1
    assert np.array_equal(_first_occurrence(X).astype(np.int64), int_form)


@pytest.mark.parametrize("fname,bio", ONE_LINE)
def test_encoder_plm_table_matches_plm_reader(fname, bio):
    path = os.path.join(DATA, fname)
    with open(path) as fh:
        lines = [ln.strip() for ln in fh if ln.strip() and not ln.startswith(">")]
    L = len(lines[0])
    X = _lib.encode_sequences(lines, _bio(bio), L, 0)
    assert X.shape[0] == len(lines)
    rows, raw = _lib.read_msa(path, _bio(bio), L)
    assert raw == len(lines)
    assert np.array_equal(_first_occurrence(X), rows)


def test_encoder_keeps_duplicates_and_order():
    seqs = ["ACGU-", "acgu-", "UUUUU", "ACGU-"]
    X = _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_RNA, 5, 0)
    assert X.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [3, 3, 3, 3, 3], [0, 1, 2, 3, 4]]
    assert _lib.encode_sequences([], _lib.DCA_BIOMOLECULE_RNA, 5, 1).shape == (0, 5)


@pytest.mark.parametrize("table", [0, 1])
def test_encoder_wrong_length(table):
    with pytest.raises(_lib.EncodeError) as ei:
        _lib.encode_sequences(["ACGU", "ACG", "ACGUA"], _lib.DCA_BIOMOLECULE_RNA, 4, table)
    assert ei.value.code == _lib.DCA_ERR_ARG and ei.value.record == 1


def test_encoder_rejected_character_plm_table_only():
    seqs = ["ACDEF", "ACDEF", "AC1EF"]
    with pytest.raises(_lib.EncodeError) as ei:
        _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_PROTEIN, 5, 0)
    assert ei.value.code == _lib.DCA_ERR_RESIDUE and ei.value.record == 2
    X = _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_PROTEIN, 5, 1)       # the mf table maps it to the gap
    assert X[2].tolist() == [0, 1, 20, 3, 4]
    # the plm RNA table: T and other capitals are the gap, digits are rejected
    assert _lib.encode_sequences(["ACGT"], _lib.DCA_BIOMOLECULE_RNA, 4, 0).tolist() == [[0, 1, 2, 4]]
    with pytest.raises(_lib.EncodeError):
        _lib.encode_sequences(["ACG7"], _lib.DCA_BIOMOLECULE_RNA, 4, 0)


def test_encoder_bad_record_via_c_abi():
    import ctypes as C
    blob = b"ACGUACGAC"
    offs = np.array([0, 4, 9], dtype=np.int32)
    out = np.zeros((2, 4), dtype=np.uint8)
    bad = C.c_int(-7)
    rc = _lib.lib().dca_encode_sequences(blob, _lib._ptr(offs), 2, _lib.DCA_BIOMOLECULE_RNA, 1, 4, _lib._ptr(out), C.byref(bad))
    assert rc == _lib.DCA_ERR_ARG and bad.value == 1
    rc = _lib.lib().dca_encode_sequences(blob, _lib._ptr(offs), 1, _lib.DCA_BIOMOLECULE_RNA, 1, 4, _lib._ptr(out), None)
    assert rc == _lib.DCA_OK
    rc = _lib.lib().dca_encode_sequences(blob, _lib._ptr(offs), 1, _lib.DCA_BIOMOLECULE_RNA, 2, 4, _lib._ptr(out), C.byref(bad))
    assert rc == _lib.DCA_ERR_ARG and bad.value == -1


def test_query_codes_names_record():
    class Boom(Exception):
        pass
    with pytest.raises(Boom, match="record 3"):
        _potts.query_codes(["ACGU", "ACGU", "AC"], _lib.DCA_BIOMOLECULE_RNA, 4, 1, Boom)


def test_writer_energies_layout(tmp_path):
    path = str(tmp_path / "PLMDCA_energies_x.txt")
    e = np.array([-1.25, 3.0e-17, 12345.678901234567])
    dca_utilities.write_sequence_energies(path, e, metadata=["# PARAMETERS USED FOR THIS COMPUTATION: "], query_file="q.fa")
    lines = open(path).read().splitlines()
    assert lines[0] == "#" + "=" * 70
    body = [ln for ln in lines if not ln.startswith("#")]
    assert len(body) == 3
    rec = [int(ln.split()[0]) for ln in body]
    val = np.array([float(ln.split()[1]) for ln in body])
    assert rec == [1, 2, 3] and np.array_equal(val, e)            # exact round trip


def test_writer_mutation_effects_layout(tmp_path):
    path = str(tmp_path / "MFDCA_mutation_effects_x.txt")
    dE = np.arange(3 * 5, dtype=np.float64).reshape(3, 5) / 7.0
    letters = _potts.state_letters(_lib.DCA_BIOMOLECULE_RNA)
    dca_utilities.write_mutation_effects(path, dE, ["A", "-", "U"], letters, metadata=None)
    body = [ln.split() for ln in open(path).read().splitlines() if not ln.startswith("#")]
    assert len(body) == 15
    assert [int(r[0]) for r in body] == [i + 1 for i in range(3) for _ in range(5)]
    assert [r[1] for r in body] == ["A"] * 5 + ["-"] * 5 + ["U"] * 5
    assert [r[2] for r in body] == letters * 3
    assert np.array_equal(np.array([float(r[3]) for r in body]).reshape(3, 5), dE)
