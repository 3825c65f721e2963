"""The two Gram sums (csim_ensemble_gram, csim_ensemble_obs_gram) at the seams of the geometry they share
(csrc/gram_plan.hpp): the upper triangle of a matrix of `cols` columns is cut into nblk (nblk + 1) / 2 blocks of 4 x 4
pairs, dealt to workgroups of 256 lanes with 1, 2 or 4 blocks per lane.  The column counts sit on both sides of the
steps nblk 1 -> 2 (4, 5) and of the block counts 253 -> 276 (88, 89: one workgroup -> two with one block per lane),
496 -> 528 (124, 125: with two) and 990 -> 1035 (176, 177: with four), and of 1035 -> 1081 (180, 181).  cols = M for the
ensemble's Gram matrix and M + 1 for the observation-space one.  65 rows (a 5 x 13 grid, 65 point observations): two
segments, the second of one row.  Every form, bit for bit the numpy restatements (tests/espace_restatement.py,
tests/etkf_restatement.py), which do not know the forms."""
import numpy as np
import pytest

import espace_restatement as espace
import etkf_restatement as etkf
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

NX, NY = 5, 13
COLS = [4, 5, 88, 89, 124, 125, 176, 177, 180, 181]
FORMS = (1, 2, 3, 0)


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def symmetric(A):
    return np.array_equal(A.view(np.int64), A.T.copy().view(np.int64))


@pytest.mark.parametrize("cols", COLS)
def test_gram_at_the_block_seams(csim, cols):
    M = cols
    X = espace.members(M, NX, NY, seed=21)
    assert espace.gram_plan(M, NX, NY) == csim.ensemble_gram_plan(M, NX, NY) == (2, 2)
    want = {c: espace.gram(X, None, c) for c in (1, 0)}
    ens = csim.Ensemble(M, NX, NY, bc=csim.bc_codes("dddd"))
    ens.upload_all(X)
    for form in FORMS:
        ens.set_option("gram_form", form)
        for c in (1, 0):
            G = ens.gram(centered=bool(c))
            assert exact_bits(G, want[c]) and symmetric(G), (form, c)
    ens.close()


@pytest.mark.parametrize("cols", COLS)
def test_obs_gram_at_the_block_seams(csim, cols):
    M, nobs = cols - 1, NX * NY
    rng = np.random.default_rng([22, cols])
    X = 3.0 + rng.standard_normal((NY + 2, NX + 2))[None] + 0.5 * rng.standard_normal((M, NY + 2, NX + 2))
    e = rng.permutation(nobs)  # every cell once: with loc < dx / 2 the plan is one level in input order
    i, j = (e % NX + 1).astype(np.int32), (e // NX + 1).astype(np.int32)
    r = rng.uniform(0.5, 2.0, nobs)
    y = 3.0 + rng.standard_normal(nobs)
    assert csim.obs_gram_plan(M, nobs) == etkf.gram_plan(M, nobs) == (2, 2)
    A, ll, n = etkf.obs_gram(X[:, j, i], y, r, True, np.arange(nobs), loglik=True)
    ens = csim.Ensemble(M, NX, NY, 1.0, 1.0, csim.bc_codes("dddd"), 0.5)
    ens.upload_all(X)
    net = ens.obs_network(i, j, r, 0.4)
    assert (net.info.lx, net.info.ly, net.info.nlevels) == (0, 0, 1)
    net.set_values(y)
    for form in FORMS:
        ens.set_option("obs_gram_form", form)
        got = ens.obs_gram(net, loglik=True)
        assert exact_bits(got.A, A) and exact_bits(got.loglik, ll) and got.n_used == n == nobs, form
        assert symmetric(got.A)
        bare = ens.obs_gram(net)
        assert bare.loglik is None and exact_bits(bare.A, A) and bare.n_used == nobs, form
    ens.close()
