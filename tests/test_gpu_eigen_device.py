"""The device eigensolver (csim_sym_eigen_batch_gpu) against the host's round-robin order
(csim_sym_eigen_ordered(CSIM_EIGEN_ROUND_ROBIN), pinned by tests/test_eigen_rr_host.py) bit for bit: single matrices at
the sizes where the pairing, the lanes of a step and the storage form change, every storage form, and batches whose
matrices differ, with a diagonal, a rank-1 and a non-finite matrix among them.  Sweep counts and statuses are the
host's.  Every test here needs the new entry points."""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def gram(n, seed):
    rng = np.random.default_rng([seed, n])
    B = rng.standard_normal((n, n + 3))
    return B @ B.T


_host = {}


def host(csim, A, key):
    """the host's result for a matrix, computed once per key"""
    if key not in _host:
        _host[key] = csim.sym_eigen(A, order="round_robin")
    return _host[key]


def check(csim, got, b, A, key):
    want = host(csim, A, key)
    assert got.status[b] == csim.EIGEN_OK and got.sweeps[b] == want.sweeps, (key, got.sweeps[b], want.sweeps)
    assert np.array_equal(bits(got.lambda_[b]), bits(want.lambda_)), key
    assert np.array_equal(bits(got.V[b]), bits(want.V)), key


def boundaries(csim):
    return [csim.sym_eigen_device_form(1, form)[1] for form in (1, 2)]


def test_single_matrices_at_every_seam(csim):
    sizes = {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256}
    for b in boundaries(csim):
        sizes |= {b - 1, b, b + 1}
    for n in sorted(sizes):
        A = gram(n, 1)
        got = csim.sym_eigen_batch(A[None])
        check(csim, got, 0, A, ("gram", n))
        assert n == 1 or 0 < got.sweeps[0] < csim.SYM_EIGEN_MAX_SWEEPS


def test_every_form_gives_the_host_bits(csim):
    for form in (1, 2, 3):
        most = csim.sym_eigen_device_form(1, form)[1]
        # form 3 admits 256, which test_single_matrices_at_every_seam runs in that form (one case of 256 is enough)
        for n in (5, 64, most if form < 3 else 129):
            assert csim.sym_eigen_device_form(n, form)[0] == form
            A = gram(n, 1)
            check(csim, csim.sym_eigen_batch(A[None], form=form), 0, A, ("gram", n))
        if form < 3:
            with pytest.raises(csim.CsimError):
                csim.sym_eigen_batch(np.eye(most + 1)[None], form=form)


def special(n, kind, seed):
    if kind == "diagonal":
        return np.diag(np.random.default_rng([seed, n, 1]).standard_normal(n))
    u = np.random.default_rng([seed, n, 2]).standard_normal(n)
    return np.outer(u, u)


@pytest.mark.parametrize("n,batch", [(8, 257), (65, 3)])
def test_batches_of_different_matrices(csim, n, batch):
    A = np.stack([gram(n, 100 + b) for b in range(batch)])
    where = {"diagonal": 1, "rank1": batch - 1, "nan": batch // 2} if batch > 3 else {"diagonal": 0, "rank1": 1, "nan": 2}
    A[where["diagonal"]] = special(n, "diagonal", 7)
    A[where["rank1"]] = special(n, "rank1", 7)
    A[where["nan"]][0, n - 1] = np.nan
    got = csim.sym_eigen_batch(A)
    for b in range(batch):
        if b == where["nan"]:
            assert got.status[b] == csim.EIGEN_NONFINITE and got.sweeps[b] == 0
            assert np.isnan(got.lambda_[b]).all() and np.isnan(got.V[b]).all()
            with pytest.raises(csim.CsimError):
                csim.sym_eigen(A[b], order="round_robin")
            continue
        check(csim, got, b, A[b], ("batch", n, b))
    assert got.sweeps[where["diagonal"]] == 0
    if batch > 3:
        assert len(set(got.sweeps.tolist())) > 2  # the workgroups of a batch stop each at its own sweep


def test_a_non_finite_entry_below_the_diagonal_counts_as_on_the_host(csim):
    A = np.stack([gram(6, 1), gram(6, 2)])
    A[1][4, 1] = np.inf
    got = csim.sym_eigen_batch(A)
    assert got.status.tolist() == [csim.EIGEN_OK, csim.EIGEN_NONFINITE]
    check(csim, got, 0, A[0], ("gram", 6))


def test_argument_errors(csim):
    for bad in (np.empty((1, 0, 0)), np.zeros((1, 257, 257))):
        with pytest.raises(csim.CsimError):
            csim.sym_eigen_batch(bad)
    with pytest.raises(csim.CsimError):
        csim.sym_eigen_batch(np.eye(3)[None], form=4)
