"""The gather and the staging that K20, K28, K29 and K30 share (csrc/packed_dev.h), checked against each other: the four
kernels on ONE input through their public wrappers.  Their own test files compare every integer with a numpy restatement;
here the kernels must agree among themselves about which structures are bad and how many pairs a good one has."""
import numpy as np
import pytest

from coarsegrainingvae_amd import contacts, distmat, lddt, pairdist

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, M = 9, 65                           # one past the chunk of 8 structures; one past a row tile of 64 atoms, across a word edge


def test_the_four_pair_kernels_agree_on_bad_structures_and_on_the_number_of_pairs():
    xyz = np.random.default_rng(965).uniform(0.0, 30.0, size=(S, M, 3)).astype(np.float32)
    xyz[3, 40, 1] = np.nan
    sel, none = np.arange(M), np.zeros((M, M), dtype=bool)
    want = np.arange(S) == 3
    k20 = contacts.contact_counts(xyz, sel, device=DEV)
    k28 = lddt.count_pairs(xyz, xyz[:1], np.zeros(S, dtype=np.int32), sel, none, none, np.ones(M, dtype=np.float32), device=DEV)
    k29 = pairdist.count_pairs(xyz, sel, np.zeros(M, dtype=np.int32), 1, none, r_max=20.0, n_bins=100, device=DEV)
    k30 = distmat.moments(xyz, sel, center=None, mask=None, device=DEV)       # no centre: zeros; no mask: every pair i < j
    for name, res in (("K20", k20), ("K28", k28), ("K29", k29), ("K30", k30)):
        assert res["bad"].dtype == np.bool_ and np.array_equal(res["bad"], want), name
        assert res["n_good"] == S - 1, name
    in_range, beyond = int(k29["hist"].sum()), int(k29["beyond"].sum())
    assert in_range > 0 and beyond > 0                                         # a 30 A box against r_max = 20 A has both
    assert k30["n_pairs"] == M * (M - 1) // 2
    assert in_range + beyond == k30["n_good"] * k30["n_pairs"] == (S - 1) * M * (M - 1) // 2
    # what the bad structure gets from each: counted nowhere
    assert k20["n_contacts"][3] == -1 and (k28["struct_counts"][3] == -1).all() and k30["dev2"][3] == 0
    assert (k20["n_contacts"][~want] >= 0).all() and (k28["struct_counts"][~want] >= 0).all() and (k30["dev2"][~want] > 0).all()
