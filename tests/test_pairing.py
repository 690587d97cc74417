"""IterativePairing, match_partners and the two sub-commands on the GPU against the numpy loop of
tests/interaction_reference.py on the planted data of tests/test_pairing_host.py.  The GPU fit is within 1e-9 of numpy, so the
comparison is made where the restatement's own margins hold (test_pairing_host.margins: the smallest gap in a species and the gap
difference across the selection boundary, each >= 1e-6 max |E|); at most 5 % of the species-rounds may be excluded."""
import os

import numpy as np
import pytest

from conftest import data_file
from pydca_amd import _lib, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.pairing import IterativePairing, IterativePairingException
from pydca_amd.plmdca.plmdca import PlmDCA
import interaction_reference as R
from test_pairing_host import MAX_EXCLUDED, margins
from test_potts_sampling import plm_model

pytestmark = pytest.mark.gpu
LETTERS = "ACGU-"


def strings(X):
    return ["".join(LETTERS[c] for c in row) for row in X]


def compare_with_reference(ip_out, ref, species_a, n_species):
    """the pairing of every species (final round) and the selected set of every round, where the margins hold"""
    hist, rhist = ip_out["history"], ref["history"]
    assert len(hist) == len(rhist)
    ok_species, ok_boundary = margins(rhist, n_species)
    excluded = sum(not v for row in ok_species for v in row) + sum(n_species for v in ok_boundary if not v)
    assert excluded <= MAX_EXCLUDED * n_species * len(rhist), excluded
    clear = True                                   # until a boundary is unclear the two runs train on the same sets
    for k, (rec, rrec) in enumerate(zip(hist, rhist)):
        if not clear:
            break
        assert rec["training_size"] == rrec["training_size"]
        assert set(rec["selected"]) == set(rrec["training"]), k
        clear = ok_boundary[k]
    if clear:                                      # the final pairing, species by species (ref's species order: first appearance)
        species = list(dict.fromkeys(species_a.tolist()))
        got, want = {}, {}
        for a, b in ip_out["pairs"]:
            got.setdefault(species_a[a], set()).add((int(a), int(b)))
        for a, b in ref["pairs"]:
            want.setdefault(species_a[a], set()).add((int(a), int(b)))
        for g, s in enumerate(species):
            if ok_species[-1][g]:
                assert got.get(s, set()) == want.get(s, set()), s
    return excluded


@pytest.fixture(scope="module")
def planted():
    return R.planted_pairs()


def test_iterative_pairing_follows_the_restatement(planted):
    XA, XB, sa, sb, tb = planted
    truth = list(enumerate(tb.tolist()))
    ip = IterativePairing(strings(XA), strings(XB), sa.tolist(), sb.tolist(), "rna", n_increment=32, seed=0)
    out = ip.run(true_pairs=truth)
    ref = R.ipa_reference(XA, XB, sa, sb, 5, n_increment=32, seed=0, true_pairs=truth)
    excluded = compare_with_reference(out, ref, sa, 80)
    print("rounds %d, excluded species-rounds %d, true-positive fraction %s" % (
        len(out["history"]), excluded, ["%.3f" % r["true_positive_fraction"] for r in out["history"]]))
    assert out["history"][-1]["true_positive_fraction"] >= out["history"][0]["true_positive_fraction"]
    assert out["pairs"].shape == (320, 2) and np.all(out["gaps"][:-1] >= out["gaps"][1:])
    # the same result for the same seed; another seed starts elsewhere
    again = IterativePairing(strings(XA), strings(XB), sa.tolist(), sb.tolist(), "rna", n_increment=32, seed=0).run(max_rounds=2)
    assert [r["selected"] for r in again["history"]] == [r["selected"] for r in out["history"][:2]]
    other = IterativePairing(strings(XA), strings(XB), sa.tolist(), sb.tolist(), "rna", n_increment=32, seed=1).run(max_rounds=1)
    assert other["history"][0]["selected"] != out["history"][0]["selected"]
    # the final model stays available: inter-protein contact scores
    scores = ip.model_context.mf_scores(True)
    assert scores.shape == (13 * 12 // 2,) and np.all(np.isfinite(scores))
    ip.model_context.close()


def test_training_set_rectangular_blocks_one_sided_species_and_duplicates():
    sizes_b = [4 + (g % 3) for g in range(30)]
    XA, XB, sa, sb, tb = R.planted_pairs(G=30, sizes_b=sizes_b, seed=5)
    truth = list(enumerate(tb.tolist()))
    train = [(a, b) for a, b in truth if sa[a] < 20]
    ref = R.ipa_reference(XA, XB, sa, sb, 5, training_pairs=train, n_increment=16, true_pairs=truth, max_rounds=3)
    # a species on the A side only, one on the B side only, and a duplicated A row (kept: it is a row of its own)
    A2 = np.concatenate([XA, XA[:2], XA[5:6]])
    sa2 = sa.tolist() + ["only_a", "only_a", int(sa[5])]
    B2 = np.concatenate([XB, XB[:3]])
    sb2 = sb.tolist() + ["only_b"] * 3
    ip = IterativePairing(strings(XA), strings(XB), sa.tolist(), sb.tolist(), "rna", training_pairs=train, n_increment=16)
    out = ip.run(max_rounds=3, true_pairs=truth)
    compare_with_reference(out, ref, sa, 30)
    assert len(out["pairs"]) == 40 and ip.dropped_species == []      # the 20 trained species' rows leave the testing set
    assert all(sa[a] >= 20 for a, _ in out["pairs"])
    ip.model_context.close()
    ip2 = IterativePairing(strings(A2), strings(B2), sa2, sb2, "rna", training_pairs=train, n_increment=16)
    assert ip2.dropped_species == ["only_a", "only_b"] and ip2.XA.shape[0] == XA.shape[0] + 3
    out2 = ip2.run(max_rounds=1)
    # the copy of A row 5 is a row of its own: not in a training pair, it takes the one B row of its species that is free
    assert len(out2["pairs"]) == 41 and XA.shape[0] + 2 in {int(a) for a, _ in out2["pairs"]}
    assert not ({int(a) for a, _ in out2["pairs"]} & {XA.shape[0], XA.shape[0] + 1})
    ip2.model_context.close()
    with pytest.raises(IterativePairingException):
        IterativePairing(strings(XA), strings(XB), ["x"] * XA.shape[0], ["y"] * XB.shape[0], "rna")
    with pytest.raises(IterativePairingException):
        IterativePairing(strings(XA), strings(XB), sa.tolist()[:-1], sb.tolist(), "rna")


def test_match_partners_on_plmdca():
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = PlmDCA(path, "protein", seqid=0.8, lambda_h=1.0, lambda_J=5.0, max_iterations=5)
    L = inst.sequences_len
    LA = L // 2
    recs = [s.replace(".", "-") for s in seqs[:18]]
    A, B = [s[:LA] for s in recs], [s[LA:] for s in recs[::-1]]
    species_a = ["s%d" % (k // 4) for k in range(18)]          # four species of 4 and one of 2
    species_b = species_a[::-1]
    res = inst.match_partners(A, B, LA, species_a, species_b)
    blocks = inst.compute_interaction_energies(A, B, LA, species_a, species_b)
    dense = inst.compute_interaction_energies(A, B, LA)
    assert dense.shape == (18, 18) and blocks["species"] == ["s0", "s1", "s2", "s3", "s4"]
    # the restatement on the fitted parameters and on codes encoded here, with the groups laid out here
    _h, Jp = plm_model(inst._fitted_context().plm_get_x(np.float32), L, 21)
    XA, XB = _lib.encode_sequences(A, _lib.DCA_BIOMOLECULE_PROTEIN, LA, 0), _lib.encode_sequences(B, _lib.DCA_BIOMOLECULE_PROTEIN, L - LA, 0)
    names = ["s0", "s1", "s2", "s3", "s4"]
    rows_a = [np.array([k for k in range(18) if species_a[k] == s]) for s in names]
    rows_b = [np.array([k for k in range(18) if species_b[k] == s]) for s in names]
    assert dense.tobytes() == R.interaction_energies(Jp, L, LA, XA, XB, 1).tobytes()
    assert inst.compute_interaction_energies(A, B, LA, gauge="as_stored").tobytes() == R.interaction_energies(Jp, L, LA, XA, XB, 0).tobytes()
    oa, ob = R.offsets_of([(len(a), len(b)) for a, b in zip(rows_a, rows_b)])
    ref_blocks = R.interaction_energies(Jp, L, LA, XA[np.concatenate(rows_a)], XB[np.concatenate(rows_b)], 1, oa, ob)
    want = []
    for g, (s, ra, rb, E) in enumerate(zip(blocks["species"], blocks["rows_a"], blocks["rows_b"], blocks["energies"])):
        assert np.array_equal(ra, rows_a[g]) and np.array_equal(rb, rows_b[g])
        assert E.tobytes() == ref_blocks[g].tobytes()
        cols, _t, gaps = R.brute_assign_with_gaps(E)
        want += [(int(ra[k]), int(rb[cols[k]]), float(E[k, cols[k]]), float(gaps[k]), s) for k in range(len(ra))]
    want = R.rank_pairs(want)
    assert [tuple(p) for p in res["pairs"].tolist()] == [(t[0], t[1]) for t in want]
    assert res["energies"].tolist() == [t[2] for t in want] and res["species"] == [t[4] for t in want]
    assert np.allclose(res["gaps"], [t[3] for t in want], rtol=0, atol=1e-12 * np.abs(dense).max())


def test_sub_commands_write_their_files(tmp_path):
    XA, XB, sa, sb, tb = R.planted_pairs(G=12, seed=3)
    fa, fb = tmp_path / "protA.fa", tmp_path / "protB.fa"
    fa.write_text("".join(">a%d\n%s\n" % (k, s) for k, s in enumerate(strings(XA))))
    fb.write_text("".join(">b%d\n%s\n" % (k, s) for k, s in enumerate(strings(XB))))
    la, lb = tmp_path / "A_species.txt", tmp_path / "B_species.txt"
    la.write_text("".join("sp%d\n" % s for s in sa))
    lb.write_text("".join("sp%d\n" % s for s in sb))
    out = str(tmp_path / "out")
    pairs_path, hist_path = mfdca_main.run_meanfield_dca(["pair_partners", "rna", str(fa), str(fb), "--species_a", str(la), "--species_b", str(lb),
                                                          "--n_increment", "16", "--seed", "2", "--output_dir", out])
    assert os.path.basename(pairs_path) == "MFDCA_partner_pairs_protA_protB.txt"
    rows = [ln.split("\t") for ln in open(pairs_path).read().splitlines() if not ln.startswith("#")]
    assert len(rows) == 48 and {r[0] for r in rows} == {"a%d" % k for k in range(48)} and {r[1] for r in rows} == {"b%d" % k for k in range(48)}
    gaps = [float(r[3]) for r in rows]
    assert gaps == sorted(gaps, reverse=True)
    assert all(r[2] == "sp%d" % sa[int(r[0][1:])] == "sp%d" % sb[int(r[1][1:])] for r in rows)
    hist = [ln.split("\t") for ln in open(hist_path).read().splitlines() if not ln.startswith("#")]
    assert [int(h[1]) for h in hist] == [48, 16, 32, 48]
    # compute_interaction_energies on both command lines: the model is fitted on the concatenated alignment
    truth = tb.tolist()
    cat = tmp_path / "cat.fa"
    cat.write_text("".join(">c%d\n%s%s\n" % (k, a, strings(XB[truth[k]:truth[k] + 1])[0]) for k, a in enumerate(strings(XA))))
    common = ["--query_file_a", str(fa), "--query_file_b", str(fb), "--split", "6", "--species_a", str(la), "--species_b", str(lb), "--output_dir", out]
    f_mf = mfdca_main.run_meanfield_dca(["compute_interaction_energies", "rna", str(cat)] + common)
    f_plm = plmdca_main.run_plm_dca(["compute_interaction_energies", "rna", str(cat), "--max_iterations", "5"] + common)
    assert os.path.basename(f_mf) == "MFDCA_interaction_energies_cat.txt" and os.path.basename(f_plm) == "PLMDCA_interaction_energies_cat.txt"
    for f in (f_mf, f_plm):
        rows = [ln.split("\t") for ln in open(f).read().splitlines() if not ln.startswith("#")]
        assert len(rows) == 12 * 16 and all(np.isfinite(float(r[3])) for r in rows)
        assert all(sa[int(r[0]) - 1] == sb[int(r[1]) - 1] for r in rows)
    # the written mean-field energies are those of the class on the same files (its own check: test_match_partners_on_plmdca)
    from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
    got = MeanFieldDCA(str(cat), "rna").compute_interaction_energies(str(fa), str(fb), 6, ["sp%d" % s for s in sa], ["sp%d" % s for s in sb])
    rows = [ln.split("\t") for ln in open(f_mf).read().splitlines() if not ln.startswith("#")]
    flat = [float(E[k, l]) for E in got["energies"] for k in range(E.shape[0]) for l in range(E.shape[1])]
    assert [float(r[3]) for r in rows] == flat
