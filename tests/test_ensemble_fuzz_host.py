"""What the batched stepper's seeded fuzz (tests/test_gpu_ensemble_fuzz.py) reaches, checked on the CPU: the case
generator is a pure function of the seed, so the default seed's cases can be classified by the pass plan, the sign
class and the edge bodies csim_ensemble_run would pick for them, without a GPU."""
import pytest

from __graft_entry__ import load_package
from ensemble_fuzz_cases import (CHUNK_CASES, DEFAULT_SEED, STRIDE, chunk_rows, div_mode, fuzz_cases)


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


@pytest.fixture(scope="module")
def reached(csim):
    T = csim.ensemble_plan(0, 512, 512)[0]
    r = dict(T=T, classes=set(), right=set(), single_strip=0, sides=set(), depth1=0, remainders=set(),
             fused_2c_off=0, rows=set(), values=set(), splits=0, big_B=0, odd_wide_passes=0)
    for c in fuzz_cases(DEFAULT_SEED):
        nx, ny = c["nx"], c["ny"]
        for s, k in enumerate(c["bc"]):
            r["sides"].add((s, k))
        r["values"].add(repr(c["value"]))
        r["splits"] += len(c["calls"]) > 1
        r["big_B"] += c["B"] > 24
        mode = div_mode(c["dx"], c["dy"])
        fused = False
        for n in c["calls"]:
            depth, q, rem = csim.ensemble_plan(n, nx, ny, c["fuse"])
            if n > 0 and depth == 1:
                r["depth1"] += 1
            if q >= 1:
                fused = True
                if rem:
                    r["remainders"].add(rem)
        if not fused:
            continue
        counts = {}
        for (D, dt, vx, vy) in c["phys"]:
            cls = csim.ensemble_sign_class(D, dt, vx, vy, c["dx"], c["dy"], c["fused_2c"])
            r["classes"].add((mode, cls))
            counts[cls] = counts.get(cls, 0) + 1
        for n_cls in counts.values():
            r["rows"].add(chunk_rows(n_cls, nx, ny, T))
        if nx > STRIDE[T]:
            r["right"].add((c["bc"][1], nx & 1))
            r["odd_wide_passes"] += nx & 1
        else:
            r["single_strip"] += 1
        r["fused_2c_off"] += c["fused_2c"] == 0
    return r


def test_generator_is_a_pure_function_of_the_seed():
    a, b = fuzz_cases(DEFAULT_SEED, 40), fuzz_cases(DEFAULT_SEED, 40)
    assert repr(a) == repr(b)
    assert repr(fuzz_cases(DEFAULT_SEED + 1, 40)) != repr(a)
    for c in a:
        assert 1 <= c["B"] <= 70 and c["nx"] >= 1 and c["ny"] >= 1 and sum(c["calls"]) == c["steps"]
        assert len(c["phys"]) == c["B"]


def test_every_sign_class_of_every_division_mode(reached):
    want = {(m, k) for m in (0, 1) for k in range(9)} | {(2, k) for k in (0, 1, 3, 4)}
    assert reached["classes"] == want, sorted(want - reached["classes"])


def test_every_right_edge_body_at_two_strips_or_more(reached):
    # col_case 3 (Dirichlet / Periodic, even nx), 4 (odd), 5 (Neumann, even), 6 (odd) — each BC kind with each parity
    assert reached["right"] == {(k, p) for k in "dnp" for p in (0, 1)}
    assert reached["odd_wide_passes"] >= 20
    assert reached["single_strip"] >= 10


def test_every_bc_kind_on_every_side(reached):
    assert reached["sides"] == {(s, k) for s in range(4) for k in "dnp"}


def test_depth_one_remainders_fused_2c_off_values_splits(reached):
    assert reached["depth1"] >= 10
    assert reached["remainders"] == set(range(1, reached["T"]))
    assert reached["fused_2c_off"] >= 10
    assert reached["values"] == {"0.0", "-0.0", "1.5"}
    assert reached["splits"] >= 50 and reached["big_B"] >= 10


def test_chunk_heights(csim, reached):
    """the fuzz mostly reaches short chunks; the targeted cases of the GPU test reach the tall ones and the clip"""
    T = reached["T"]
    assert len(reached["rows"]) >= 2
    assert T == 4, "the targeted chunk heights are worked out for pass depth 4"
    rows = [chunk_rows(B, nx, ny, T) for B, nx, ny, _ in CHUNK_CASES]
    assert rows == [12, 18, 36, 66, 5, 4]
    for B, nx, ny, steps in CHUNK_CASES:
        assert csim.ensemble_plan(steps, nx, ny)[1] >= 1  # at least one multi-step pass

