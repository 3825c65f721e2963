"""tests/held_restatement.py pinned without a GPU: the slots that occur against a brute-force mask and against the
library's own bookkeeping rule (csim_obs_slots_present, host-only), its error cases; the row transform against a
scalar walk through the text of csim_ensemble_transform(centered = 1) for one cell; the row mv against mv of
csim_ensemble_relax as tests/relax_restatement.py states it.  Bits are compared through integer views."""
import numpy as np
import pytest

import held_restatement as held
import relax_restatement as relax
from __graft_entry__ import load_package

ERR_ARG = 1


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def brute(slot):
    return sum(1 << s for s in range(held.MAX_SLOTS) if any(int(v) == s for v in slot))


def test_slots_present_is_the_brute_force_mask(csim):
    assert csim.OBS_MAX_SLOTS == held.MAX_SLOTS == 64
    rng = np.random.default_rng(1)
    cases = [[0], [63], [5, 5, 5], list(range(64)), list(range(63, -1, -1)) + [7, 7], [0, 2, 4, 63],
             rng.integers(0, 64, 200).tolist(), rng.integers(10, 20, 31).tolist()]
    for slot in cases:
        want = brute(slot)
        assert held.slots_present(slot) == want == csim.obs_slots_present(slot), slot
    assert brute(list(range(64))) == (1 << 64) - 1
    # a slot that does not occur has no bit
    assert held.slots_present([0, 2, 4, 63]) >> 3 & 1 == 0 and csim.obs_slots_present([0, 2, 4, 63]) >> 3 & 1 == 0
    # no slots given: every observation in slot 0
    assert held.slots_present(None) == csim.obs_slots_present(None) == csim.obs_slots_present(None, 17) == 1


def test_slots_present_errors(csim):
    for bad in ([-1], [64], [0, 1, 64], [3, -2, 3], [1 << 20]):
        with pytest.raises(ValueError):
            held.slots_present(bad)
        with pytest.raises(csim.CsimError) as ei:
            csim.obs_slots_present(bad)
        assert ei.value.code == ERR_ARG
    import ctypes
    L = csim.lib()
    m = ctypes.c_ulonglong(77)
    one = (ctypes.c_int * 1)(3)
    assert L.csim_obs_slots_present(0, one, ctypes.byref(m)) == ERR_ARG
    assert L.csim_obs_slots_present(1, one, None) == ERR_ARG
    bad = (ctypes.c_int * 2)(3, 64)
    assert L.csim_obs_slots_present(2, bad, ctypes.byref(m)) == ERR_ARG and m.value == 77   # nothing written
    assert L.csim_obs_slots_present(1, one, ctypes.byref(m)) == 0 and m.value == 8


def scalar_row(x, W, wbar):
    """one row through the text of transform(centered = 1), operation by operation on Python floats"""
    M = len(x)
    s = 0.0
    for k in range(M):
        s = s + x[k]
    m = s / M
    p = [x[k] - m for k in range(M)]
    mp = m
    if wbar is not None:
        d = 0.0
        for k in range(M):
            d = d + p[k] * wbar[k]
        mp = m + d
    out = []
    for r in range(M):
        a = 0.0
        for k in range(M):
            a = a + p[k] * W[k][r]
        out.append(mp + a)
    return out


@pytest.mark.parametrize("M", [2, 5, 65])
def test_row_transform_is_the_cell_transform_of_a_row(M):
    rng = np.random.default_rng([2, M])
    H = 3.0 + rng.standard_normal((7, M))
    W = np.eye(M) + 0.1 * rng.standard_normal((M, M))
    wbar = 0.1 * rng.standard_normal(M)
    for wb in (wbar, None):
        got = held.row_transform(H, W, wb)
        want = np.array([scalar_row(H[o].tolist(), W.tolist(), None if wb is None else wb.tolist()) for o in range(7)])
        assert exact_bits(got, want)
    # the identity without a shift keeps a row up to the rounding of (x - m) + m, and a selection resamples
    assert np.allclose(held.row_transform(H, np.eye(M)), H, rtol=1e-15, atol=0)


@pytest.mark.parametrize("M", [2, 5, 65])
def test_row_mv_is_mv_of_relax(M):
    rng = np.random.default_rng([3, M])
    H = 3.0 + rng.standard_normal((9, M))
    m, v = held.row_mv(H)
    wm, wv = relax.mv(np.ascontiguousarray(H.T))
    assert exact_bits(m, wm) and exact_bits(v, wv)
    np.testing.assert_allclose(m, H.mean(axis=1), rtol=1e-14)
    np.testing.assert_allclose(v, H.var(axis=1, ddof=1), rtol=1e-12)


def test_assemble_takes_each_row_from_its_slot():
    rng = np.random.default_rng(4)
    states = {0: rng.standard_normal((3, 6)), 2: rng.standard_normal((3, 6)), 5: rng.standard_normal((3, 6))}
    slot = [0, 2, 2, 5, 0, 5]
    H = held.assemble(states, slot, lambda s: s)
    for o, s in enumerate(slot):
        assert exact_bits(H[o], states[s][:, o])


# what tests/test_gpu_held.py allows the GPU, 8 times this, is measured here
CLAIM_REFERENCE = 1.12e-14


def test_the_claim_on_the_cpu_and_its_measured_disagreement(csim):
    """hold, run, held analysis against analysis, run, in numpy with the oracle's stepping and the restatements, over the
    32 scenarios: the largest difference relative to the RMS analysis increment is the reference's own disagreement
    (1.117e-14 when this was written), and in every scenario the analysis with rows from the wrong time is far outside
    100 x 8 x that, so the GPU test can tell the two apart"""
    import etkf_restatement as etkf
    import obsnet_restatement as obsnet
    import obsop_restatement as obsop
    from oracle import cpu_oracle as ora

    def operator(X, t, i, j, taps):
        if taps is None:
            return X[obsnet.forecast(X.shape[0], t)][:, j, i]
        return obsop.h_members(X, t, i, j, taps)

    scenarios = held.claim_scenarios()
    assert len(scenarios) == 32 and {s[1] for s in scenarios} == set(held.CLAIM_KINDS)
    worst, least = 0.0, np.inf
    for sc in scenarios:
        one, two, wrong, free = held.claim_cpu(csim, ora, etkf, operator, sc)
        worst = max(worst, held.claim_error(one, two, free, sc[2]))
        least = min(least, held.claim_error(wrong, two, free, sc[2]))
    print(f"largest disagreement {worst:.4e}, least wrong-time difference {least:.4e}")
    assert 0.0 < worst <= CLAIM_REFERENCE
    assert least > 100.0 * 8.0 * CLAIM_REFERENCE
