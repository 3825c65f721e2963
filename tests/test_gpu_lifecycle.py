"""What a handle owns and how it gives it back (csrc/owned.hpp): steppers, Fields and ensembles created, used and
closed many times over — closed with a snapshot in flight, straight after an unsynchronised run, or by __del__ alone
— in a process of its own that must end clean; and the snapshot, which travels through the same Capture as the
ensemble's diagnostics, in every exchange schedule: each snapshot is the interior at its own begin, bit for bit.
The reference is the CPU oracle (run_single, and torus_oracle of tests/test_gpu_comm.py on the self-linked tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from __graft_entry__ import load_package   # noqa: E402
from oracle import cpu_oracle as ora       # noqa: E402

pytestmark = pytest.mark.gpu

D, VX, VY, DT = 0.05, 0.5, -0.25, 0.1
ERR_STATE = 4   # CSIM_ERR_STATE (include/csim.h)
ROUNDS = 50


# ---- lifecycle ---------------------------------------------------------------------------------------------------
def _centre_rank(csim, it):
    """rank 4 of a 3 x 3 decomposition: four side and four diagonal peers, so every line and face buffer exists; in
    external-halo mode it takes its own faces back as its neighbours' (sizes of opposite directions are equal)"""
    dec = csim.decomp_init(9, 4, 192, 144)
    assert (dec.nx_local, dec.ny_local) == (64, 48) and all(n >= 0 for n in dec.nbr)
    st = csim.Stepper(dec, 1.0, 1.0, csim.bc_codes("dddd"))
    st.set_option("external_halo", 1)
    assert sum(p >= 0 for p in st.faces_neighbors(3)[0]) == 8
    st.init_gaussian(1.0, 0.1, 0.5, 0.5)
    st.faces_unpack(3, st.faces_pack(3))
    st.run(D, DT, VX, VY, 3)
    if it % 4 == 0:
        st.snapshot_begin()          # closed with the copy in flight, never waited for
        st.close()
    elif it % 4 == 1:
        st.halo_unpack(st.halo_pack())
        st.run(D, DT, VX, VY, 1)     # closed straight after an unsynchronised run
        st.close()
    elif it % 4 == 2:
        del st                       # __del__ without close
    else:
        st.snapshot_begin()
        assert st.snapshot_wait().shape == (48, 64)
        st.close()
        st.close()                   # a second close is a no-op


def _single_rank(csim, it, u0):
    st = csim.Stepper.single(130, 67, 1.0, 1.0, csim.bc_codes("dnpd"))
    st.upload(u0)
    st.run(D, DT, VX, VY, 13)
    if it % 3 == 0:
        st.snapshot_begin()
        st.run(D, DT, VX, VY, 2)
    if it % 2:
        del st
    else:
        st.close()


def _field(csim, it):
    a, b = csim.Field(130, 67), csim.Field(130, 67)
    a.fill(1.0 + it)
    b.fill(2.0)
    a.swap(b)                        # the memory changes hands: each handle gives back what it holds now
    assert a.sum() == 2.0 * 130 * 67
    del a
    assert b.sum() == (1.0 + it) * 130 * 67
    del b


def _ensemble(csim, it):
    ens = csim.Ensemble(4, 64, 48, 1.0, 1.0, csim.bc_codes("dnpd"))
    ens.set_physics(D, DT, [VX, -VX, 0.0, VX], VY)
    for m in range(4):
        ens.init_gaussian(m, 1.0 + 0.1 * m, 0.1, 0.4, 0.5)
    net = ens.obs_network([5, 20, 40], [7, 30, 44], 0.01, 4.0)
    net.observe(0, seed=it)
    ens.assimilate_network(net, truth_member=0)
    ens.run(5)
    if it % 3 == 0:
        ens.stats_begin()            # a capture in flight at the close
    if it % 2:
        net.close()
        del ens
    else:
        ens.close()                  # closes the network too
        net.close()


def _fresh_stepper_matches_oracle(csim, u0):
    bc = csim.bc_codes("dnpd")
    st = csim.Stepper.single(130, 67, 1.0, 1.0, bc)
    st.upload(u0)
    st.run(D, DT, VX, VY, 7)
    st.run(D, DT, VX, VY, 6)
    got = st.download()
    st.close()
    want = u0.copy()
    ora.run_single(want, 1.0, 1.0, D, VX, VY, DT, bc, 13)
    return np.array_equal(got, want)


def _lifecycle_main():
    csim = load_package()
    csim.lib()
    csim.set_device(0)
    rng = np.random.default_rng(50)
    u0 = rng.standard_normal((67 + 2, 130 + 2))
    for it in range(ROUNDS):
        _centre_rank(csim, it)
        _single_rank(csim, it, u0)
        _field(csim, it)
        _ensemble(csim, it)
    assert _fresh_stepper_matches_oracle(csim, u0)
    print("lifecycle ok", flush=True)


def test_handles_created_used_and_closed_fifty_times():
    """the loops above in a child process: it prints its last line and exits 0 — no abort, no fault at a close or at
    the interpreter's exit — after a fresh stepper has matched the oracle bit for bit on a 7 + 6-step run"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("lifecycle ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- snapshot ----------------------------------------------------------------------------------------------------
NX, NY, SIDES = 64, 48, (1, 1, 1, 1)


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    pkg.set_device(0)
    return pkg


@pytest.fixture(scope="module")
def torus_states(csim):
    """the seeded field on the self-linked tile and the oracle's interiors after 13 and 26 steps"""
    from test_gpu_comm import torus_oracle
    codes = csim.bc_codes("dddd")
    u0 = np.random.default_rng(13).standard_normal((NY + 2, NX + 2))
    u13 = torus_oracle(u0, 1.0, 1.0, D, VX, VY, DT, 13, SIDES, codes)
    u26 = torus_oracle(u13, 1.0, 1.0, D, VX, VY, DT, 13, SIDES, codes)
    return u0, {0: u0[1:-1, 1:-1].copy(), 13: u13[1:-1, 1:-1].copy(), 26: u26[1:-1, 1:-1].copy()}


@pytest.mark.parametrize("relay_events", [0, 1])
@pytest.mark.parametrize("relay", [1, 0])
@pytest.mark.parametrize("overlap", [0, 1, 3, 4, 5])
def test_snapshot_is_the_interior_at_its_own_begin(csim, torus_states, overlap, relay, relay_events):
    """begin, 13 steps enqueued behind it, wait: the state at the begin.  Then begin, 13 steps, begin again (it lets
    the copy in flight finish and replaces it), 13 more steps, wait: the state at the second begin.  The staging copy
    is ordered on the stream the field state is ordered on, whichever schedule moved it there."""
    from test_gpu_comm import self_neighbor_decomp
    u0, want = torus_states
    st = csim.Stepper(self_neighbor_decomp(csim, NX, NY, SIDES), 1.0, 1.0, csim.bc_codes("dddd"))
    st.comm_init(csim.comm_unique_id())
    try:
        st.set_option("overlap", overlap)
    except csim.CsimError as e:    # schedule 3 on a device without signal memory, as tests/test_gpu_relay.py
        assert overlap == 3 and e.code == ERR_STATE and "signal memory" in str(e), e
        st.close()
        return
    st.set_option("relay", relay)
    st.set_option("relay_events", relay_events)
    st.upload(u0)
    st.snapshot_begin()
    st.run(D, DT, VX, VY, 13)
    assert np.array_equal(st.snapshot_wait(), want[0])
    st.snapshot_begin()
    st.run(D, DT, VX, VY, 13)
    st.snapshot_begin()
    st.run(D, DT, VX, VY, 13)
    assert np.array_equal(st.snapshot_wait(), want[26])
    with pytest.raises(csim.CsimError):
        st.snapshot_wait()           # nothing in flight any more
    assert np.array_equal(st.download_interior(), torus_oracle_interior(csim, want, 39))
    st.close()


def torus_oracle_interior(csim, want, steps):
    """the oracle's interior after `steps` (a multiple of 13) steps, extending the module's states"""
    if steps not in want:
        from test_gpu_comm import torus_oracle
        u = np.zeros((NY + 2, NX + 2))
        u[1:-1, 1:-1] = want[steps - 13]
        want[steps] = torus_oracle(u, 1.0, 1.0, D, VX, VY, DT, 13, SIDES, csim.bc_codes("dddd"))[1:-1, 1:-1].copy()
    return want[steps]


if __name__ == "__main__":
    _lifecycle_main()
