"""Host side of the observation networks (csim_obs_network_* in include/csim.h), no GPU needed: the entry points are
declared and exported, csim_obs_noise is the stated composition of csim_philox4x32 and csim_normal_from_bits bit for
bit and apart from every stream of csim_ensemble_perturb, its deviates have the moments of a standard normal, the
restatement's chunked sums (tests/obsnet_restatement.py) give closed forms on dyadic data, and without a device nothing
can be created."""
import numpy as np
import pytest

import obsnet_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_obs_network_create": 9, "csim_obs_network_destroy": 1, "csim_obs_network_info": 5,
         "csim_obs_network_set_values": 2, "csim_obs_network_observe": 5, "csim_obs_noise": 4,
         "csim_ensemble_assimilate_network": 5, "csim_obs_network_fetch": 7, "csim_obs_network_log": 4,
         "csim_obs_network_log_reset": 1}


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
    for name, nargs in NAMES.items():
        assert name in declared
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert csim.OBS_CYCLE_FIELDS == ref.FIELDS and csim.C.sizeof(csim.CsimObsCycle) == 8 * 13
    for name in ("obs_network", "assimilate_network"):
        assert callable(getattr(csim.Ensemble, name))
    for name in ("set_values", "observe", "fetch", "log", "log_reset", "info", "close"):
        assert hasattr(csim.ObsNetwork, name)
    assert L.csim_abi_version() == 1


SEEDS = [0, 1, 2025, 0xDEADBEEFCAFEF00D, (1 << 64) - 1]
DRAWS = [0, 1, 7, (1 << 32) - 1]


def composed(csim, seed, draw, o):
    """csim_normal_from_bits(out[0] | out[1] << 32), out = csim_philox4x32((o, 0, 0xFFFFFFFF, draw), seed)"""
    out = csim.philox4x32([o, 0, 0xFFFFFFFF, draw], [seed & 0xFFFFFFFF, seed >> 32])
    return csim.normal_from_bits(int(out[0]) | (int(out[1]) << 32))


def test_noise_is_the_stated_composition(csim):
    idx = np.arange(10000)
    z = csim.obs_noise(2025, 3, idx)
    want = np.array([composed(csim, 2025, 3, int(o)) for o in idx])
    assert same_bits(z, want)
    assert same_bits(z, ref.noise(2025, 3, idx))
    edge = [0, 1, 255, 256, (1 << 20) - 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]
    for seed in SEEDS:
        for draw in DRAWS:
            got = csim.obs_noise(seed, draw, edge)
            assert same_bits(got, [composed(csim, seed, draw, o) for o in edge]), (seed, draw)
            assert same_bits(got, ref.noise(seed, draw, edge)), (seed, draw)
    # a function of all three arguments
    assert len({float(csim.obs_noise(s, d, o)) for s in (1, 2) for d in (0, 1) for o in (0, 1)}) == 8
    assert csim.lib().csim_obs_noise(1, 0, 0, None) == 1
    for bad in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 32)):
        with pytest.raises(ValueError):
            csim.obs_noise(bad[0], bad[1], 0)


def test_noise_is_apart_from_the_perturbation_streams(csim):
    """counter word 2 is 0xFFFFFFFF where csim_ensemble_perturb has the member index: for the same seed, draw and
    counter words 0 and 1 (lattice point 2 o, whose deviate is the first of its Philox call) no member 0 .. 1025 gives
    the observation's deviate"""
    for seed, draw in ((2025, 0), (SEEDS[3], 7)):
        for o in (0, 1, 4097):
            z = csim.obs_noise(seed, draw, o)
            key = [seed & 0xFFFFFFFF, seed >> 32]
            for k in range(1026):
                out = csim.philox4x32([o, 0, k, draw], key)
                assert csim.normal_from_bits(int(out[0]) | (int(out[1]) << 32)) != z, (seed, draw, o, k)


def test_noise_moments(csim):
    """N = 65536 deviates of the library, seed 2025, draw 0: the mean within 5 / sqrt(N) of 0 and the variance within
    5 sqrt(2 / N) of 1, the sampling bounds of a standard normal (five standard errors); the restatement gives the same
    bits"""
    N = 65536
    z = csim.obs_noise(2025, 0, np.arange(N))
    assert same_bits(z, ref.noise(2025, 0, np.arange(N)))
    mean, var = z.mean(), z.var(ddof=1)
    print(f"mean {mean:+.6f} (bound {5 / np.sqrt(N):.6f}), variance {var:.6f} (bound {5 * np.sqrt(2 / N):.6f})")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / N)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_chunked_sums_closed_forms(n):
    """dyadic data: every partial sum is exact, so the chunked sum is the plain sum"""
    k = np.arange(n, dtype=np.float64)
    assert ref.chunked(np.ones(n)) == n
    assert ref.chunked(k / 8.0) == n * (n - 1) / 16.0
    assert ref.chunked(k * k) == (n - 1) * n * (2 * n - 1) / 6.0
    y, hb, ha = k / 4.0, k / 8.0, k / 4.0 - 0.5
    rec = ref.cycle(y, hb, np.full(n, 2.0), ha, np.full(n, 0.5), 0.25, xt=y)
    S1, S2 = n * (n - 1) / 2.0, (n - 1) * n * (2 * n - 1) / 6.0
    want = dict(n=n, has_truth=1.0, sum_ob=S1 / 8, sum_ob2=S2 / 64, sum_oa=0.5 * n, sum_oa2=0.25 * n,
                sum_oa_ob=S1 / 16, sum_ab_ob=S2 / 64 - S1 / 16, sum_vb=2.0 * n, sum_va=0.5 * n, sum_r=0.25 * n,
                sum_eb2=S2 / 64, sum_ea2=0.25 * n)
    assert set(rec) == set(ref.FIELDS)
    for f in ref.FIELDS:
        assert rec[f] == want[f], f
    none = ref.cycle(y, hb, np.full(n, 2.0), ha, np.full(n, 0.5), 0.25)
    assert none["has_truth"] == 0.0 and none["sum_eb2"] == 0.0 and none["sum_ea2"] == 0.0
    assert not np.signbit(none["sum_eb2"]) and none["sum_ob2"] == want["sum_ob2"]


def test_chunked_sums_follow_the_chunks():
    """the order is the definition's: after 2^53 the ones of the first chunk are lost one by one, those of the second
    chunk are added up among themselves first and survive; one running sum over all terms would lose them too"""
    big = 2.0 ** 53
    t = np.concatenate(([big], np.ones(511)))
    assert ref.chunked(t) == big + 256.0
    assert float(np.add.accumulate(t)[-1]) == big
    assert ref.chunked(np.array([-0.0])) == 0.0 and not np.signbit(ref.chunked(np.array([-0.0])))


def test_null_handles_are_refused_before_the_device(csim):
    L, C = csim.lib(), csim.C
    out = C.c_void_p()
    ii, rr = (C.c_int * 1)(1), (C.c_double * 1)(1.0)
    assert L.csim_obs_network_create(None, 1, ii, ii, rr, 1.0, 0, 0, C.byref(out)) == 1 and not out.value
    assert L.csim_obs_network_create(None, 1, ii, ii, rr, 1.0, 0, 0, None) == 1
    assert L.csim_obs_network_destroy(None) == 0
    assert L.csim_obs_network_info(None, None, None, None, None) == 1
    assert L.csim_obs_network_set_values(None, rr) == 1
    assert L.csim_obs_network_observe(None, 0, 1, 0, 1) == 1
    assert L.csim_ensemble_assimilate_network(None, None, 1.0, -1, 0) == 1
    assert L.csim_obs_network_fetch(None, None, None, None, None, None, None) == 1
    assert L.csim_obs_network_log(None, 0, None, None) == 1
    assert L.csim_obs_network_log_reset(None) == 1


def test_no_cpu_fallback_without_device(csim):
    """Without a GPU there is no ensemble (csim_ensemble_create fails with CSIM_ERR_HIP), and a network needs one: with
    no ensemble handle csim_obs_network_create refuses and leaves *out null, so nothing is ever made on the host.  The
    create path behind a live ensemble cannot be reached without a device."""
    try:
        n = csim.device_count()
    except csim.CsimError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(csim.CsimError) as ei:
        csim.Ensemble(3, 8, 8)
    assert ei.value.code == 2
    e = csim.Ensemble.__new__(csim.Ensemble)   # what is left of an ensemble that could not be created
    e._h = None
    with pytest.raises(csim.CsimError) as ei:
        csim.ObsNetwork(e, [1], [1], 1.0, 2.0)
    assert ei.value.code == 1 and "null ensemble" in str(ei.value)
