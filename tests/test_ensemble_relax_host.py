"""Host side of the relaxation inflation (csim_ensemble_prior_capture / csim_ensemble_relax), no GPU needed: the two
entry points are declared and exported, the numpy restatement (tests/relax_restatement.py) gives the closed forms of the
definition exactly on dyadic data, and without a device the calls fail loudly."""
import numpy as np
import pytest

import relax_restatement as ref
from __graft_entry__ import load_package

NAMES = ["csim_ensemble_prior_capture", "csim_ensemble_relax"]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name in NAMES:
        assert name in declared
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (3 if name.endswith("capture") else 5)
    assert (csim.RELAX_SPREAD, csim.RELAX_PERT) == (1, 2) == (ref.SPREAD, ref.PERT)
    assert csim.lib().csim_abi_version() == 1


def two_members(m, a, ny=3, nx=4):
    """members m - a and m + a on every cell, ghost ring included"""
    X = np.empty((2, ny + 2, nx + 2))
    X[0], X[1] = m - a, m + a
    return X


@pytest.mark.parametrize("alpha,scale", [(1.0, 2.0), (0.5, 1.5)])
def test_rtps_closed_form(alpha, scale):
    """M = 2, members m -+ a, sb = 2 sa: f = alpha (2 sa - sa) / sa = alpha exactly, so the perturbations are scaled by
    1 + alpha; m, a powers of two, so every step is exact"""
    m, a = 4.0, 0.25
    prior, analysis = two_members(m, 2 * a), two_members(m, a)
    sb = ref.capture(prior, ref.SPREAD)
    sa = ref.capture(analysis, ref.SPREAD)
    assert same_bits(sb, 2.0 * sa) and (sa > 0).all()
    got, f = ref.relax(analysis, sb, ref.SPREAD, alpha)
    want = analysis.copy()
    want[0, 1:-1, 1:-1], want[1, 1:-1, 1:-1] = m - scale * a, m + scale * a
    assert same_bits(got, want)
    assert same_bits(f[1:-1, 1:-1], np.full((3, 4), alpha))
    ring = np.ones(f.shape, dtype=bool)
    ring[1:-1, 1:-1] = False
    assert same_bits(f[ring], np.zeros(ring.sum()))


def test_rtps_leaves_untouched_cells_and_minus_zero():
    """where the analysis left the bits alone f is exactly +0 and the cell is not written: a -0 stays a -0; where all
    members agree (sa == 0) f is +0 too; alpha == 0 changes nothing"""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((5, 6, 7))
    X[:, 2, 2] = -0.0
    X[:, 3, 3] = 1.5
    sb = ref.capture(X, ref.SPREAD)
    got, f = ref.relax(X, sb, ref.SPREAD, 1.0)
    assert same_bits(got, X) and same_bits(f, np.zeros(f.shape)) and np.signbit(got[:, 2, 2]).all()
    A = X.copy()
    A[:, 1:3, 1:4] *= 0.5
    got, f = ref.relax(A, sb, ref.SPREAD, 1.0, t=None)
    assert not same_bits(got[:, 1:3, 1:4], A[:, 1:3, 1:4])
    changed = (got.view(np.int64) != A.view(np.int64)).any(axis=0)
    assert not changed[3:, :].any() and not changed[:, 4:].any() and np.signbit(got[:, 2, 2]).all()
    got0, f0 = ref.relax(A, sb, ref.SPREAD, 0.0)
    assert same_bits(got0, A) and same_bits(f0, np.zeros(f0.shape))


def test_rtpp_closed_form_and_truth_member():
    """alpha = 1 on dyadic data: x_k + ((xb_k - m_b) - (x_k - m)) = m + (xb_k - m_b) exactly: the captured perturbations
    around the analysis mean; the truth member and the ghost ring are not touched"""
    rng = np.random.default_rng(1)
    B, t = 5, 2
    prior = rng.integers(-64, 64, (B, 5, 6)) / 8.0
    analysis = rng.integers(-64, 64, (B, 5, 6)) / 8.0
    ks = ref.forecast(B, t)
    assert ks == [0, 1, 3, 4]
    # means of four dyadic values are exact
    cap = ref.capture(prior, ref.PERT, t)
    got, f = ref.relax(analysis, cap, ref.PERT, 1.0, t)
    assert f is None
    inner = (slice(1, -1), slice(1, -1))
    m = analysis[ks].mean(axis=0)
    mb = prior[ks].mean(axis=0)
    for k in ks:
        assert same_bits(got[k][inner], (m + (prior[k] - mb))[inner])
    assert same_bits(got[t], analysis[t])
    ring = np.ones(prior.shape[1:], dtype=bool)
    ring[inner] = False
    assert same_bits(got[:, ring], analysis[:, ring])
    half, _ = ref.relax(analysis, cap, ref.PERT, 0.5, t)
    for k in ks:
        assert same_bits(half[k][inner], (analysis[k] + 0.5 * ((prior[k] - mb) - (analysis[k] - m)))[inner])


def test_null_handle_is_refused_before_the_device(csim):
    L = csim.lib()
    assert L.csim_ensemble_prior_capture(None, 1, -1) == 1
    assert L.csim_ensemble_relax(None, 1, 0.5, -1, None) == 1
    with pytest.raises(ValueError):
        csim.Ensemble.__new__(csim.Ensemble).prior_capture("no such mode")


def test_no_cpu_fallback_without_device(csim):
    """Without a GPU the ensemble cannot be created, so there is nothing to relax on the host: the calls raise"""
    try:
        n = csim.device_count()
    except csim.CsimError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(csim.CsimError):
        e = csim.Ensemble(3, 8, 8)
        e.prior_capture("spread")
        e.relax(0.5)
