"""The iterative pairing loop in numpy (tests/interaction_reference.ipa_reference: oracle mean-field fit, the float64 restatement
of the interaction energies, exhaustive assignment) on planted paired data: G = 80 species of 4 pairs, LA = 6, LB = 7, q = 5,
each B site a permuted copy of an A site with probability 0.9, 3 % gaps, from a random pairing with n_increment = 32.

A numpy prototype of this description (seeds 0 - 2) assigned 91 - 96 % of the pairs correctly in round 1 and at least 99 % by
round 5, and the smallest gap of any species was never below 7e-4 of max |E| in any round.  The generator here differs in its
random streams, so the test asserts what the issue asks of it: the final true-positive fraction is at least round 1's, and the
margin condition tests/test_pairing.py relies on (at most 5 % of the species-rounds fall below 1e-6 max |E|)."""
import numpy as np
import pytest

import interaction_reference as R

MARGIN = 1e-6
MAX_EXCLUDED = 0.05


def margins(history, n_species):
    """per round: which species have their smallest gap >= MARGIN max|E|, and whether the selection boundary is that clear"""
    ok_species, ok_boundary = [], []
    for rec in history:
        lim = MARGIN * rec["max_abs_E"]
        ok_species.append([g >= lim for g in rec["min_gap"]])
        # an exact tie across the boundary is two rows of one species that would swap partners: the solver gives both the same
        # bits (assignment.h) and the rule "equal gaps in ascending A index" decides, on any model
        ok_boundary.append(rec["boundary"] is None or rec["boundary"] == 0.0 or rec["boundary"] >= lim)
    return ok_species, ok_boundary


@pytest.fixture(scope="module")
def planted():
    return R.planted_pairs()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_ipa_on_planted_pairs(planted, seed):
    XA, XB, sa, sb, tb = planted
    truth = list(enumerate(tb.tolist()))
    out = R.ipa_reference(XA, XB, sa, sb, 5, n_increment=32, seed=seed, true_pairs=truth)
    hist = out["history"]
    tpf = [rec["true_positive_fraction"] for rec in hist]
    print("seed %d: %d rounds, true-positive fraction per round %s" % (seed, len(hist), ["%.3f" % v for v in tpf]))
    assert len(hist) == 1 + -(-320 // 32)                  # round 11 trains on all 320 assigned pairs
    assert [rec["training_size"] for rec in hist] == [320] + [min(32 * k, 320) for k in range(1, len(hist))]
    assert tpf[-1] >= tpf[0]
    assert tpf[-1] >= 0.9                                  # the planted signal is found
    assert len(out["pairs"]) == 320 and len(set(a for a, _ in out["pairs"])) == 320 and len(set(b for _, b in out["pairs"])) == 320
    assert all(sa[a] == sb[b] for a, b in out["pairs"])
    gaps = np.array(out["gaps"])
    assert np.all(gaps[:-1] >= gaps[1:]) and np.all(gaps >= 0)
    ok_species, ok_boundary = margins(hist, 80)
    small = min(min(rec["min_gap"]) / rec["max_abs_E"] for rec in hist)
    print("smallest gap of any species over all rounds: %.3g of max |E|" % small)
    excluded = sum(not v for row in ok_species for v in row)
    assert excluded <= MAX_EXCLUDED * 80 * len(hist)
    assert sum(not v for v in ok_boundary) <= MAX_EXCLUDED * len(hist)


def test_random_pairing_is_one_to_one_and_seeded(planted):
    XA, XB, sa, sb, _tb = planted
    _o, rows_a = R.group_rows(list(sa))
    _o, rows_b = R.group_rows(list(sb))
    p0, p0b, p1 = R.random_pairing(rows_a, rows_b, 0), R.random_pairing(rows_a, rows_b, 0), R.random_pairing(rows_a, rows_b, 1)
    assert p0 == p0b and p0 != p1
    assert sorted(a for a, _ in p0) == list(range(320)) and sorted(b for _, b in p0) == list(range(320))
    assert all(sa[a] == sb[b] for a, b in p0)
    # every within-species permutation is reachable: over the 80 species of 4, most of the 24 orders appear
    orders = {tuple(b - min(bs) for b in bs) for bs in ([b for _, b in p0[4 * g:4 * g + 4]] for g in range(80))}
    assert len(orders) >= 12


def test_training_set_and_rectangular_blocks():
    sizes_b = [4 + (g % 3) for g in range(30)]
    XA, XB, sa, sb, tb = R.planted_pairs(G=30, sizes_b=sizes_b, seed=5)
    assert XB.shape[0] == sum(sizes_b)
    truth = list(enumerate(tb.tolist()))
    train = [(a, b) for a, b in truth if sa[a] < 20]
    out = R.ipa_reference(XA, XB, sa, sb, 5, training_pairs=train, n_increment=16, true_pairs=truth, max_rounds=3)
    assert out["history"][0]["training_size"] == 80 and out["history"][1]["training_size"] == 96
    assert set(train) <= set(out["history"][2]["training"])
    # the rows of the training pairs leave the testing set: the 10 other species' A rows are assigned, 0 - 2 B rows of each stay free
    assert len(out["pairs"]) == 40 and all(sa[a] >= 20 for a, _ in out["pairs"])
    used_b = {b for _, b in train}
    assert not any(b in used_b for _, b in out["pairs"])
    for rec in out["history"]:
        assert len({a for a, _ in rec["training"]}) == len(rec["training"]) == len({b for _, b in rec["training"]})
    assert out["history"][-1]["true_positive_fraction"] >= 0.8
