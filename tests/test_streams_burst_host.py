"""CPU checks of the stream group's burst planner (fec_streams_plan_burst_host): the per-stream
routine fec_streams_decode_burst builds its records with -- runs of received packets on the fast
path skipped in one go, everything else stepped -- gives every packet the fate fec_plan_host gives
it, however the stream is cut into bursts.  No device work here."""
import numpy as np
import pytest

from conftest import load_pattern

import fec_erasure_code_unit_test_relay_amd as fec

L = 300
TUPLES = [(10, 3, 3), (10, 5, 2), (10, 1, 1), (3, 2, 2), (4, 4, 4)]


def synthetic_pattern(T, B, N, P=400):
    """P + T flags: runs of B erasures starting at 20, 60, 100, ... while the start is below P - 60,
    plus one run of T + N + 2 erasures at P / 2."""
    pat = np.zeros(P + T, dtype=np.uint8)
    start = 20
    while start < P - 60:
        pat[start:start + B] = 1
        start += 40
    pat[P // 2:P // 2 + T + N + 2] = 1
    return pat


def run_edges(pat):
    """First and last packet of every erasure run."""
    e = np.concatenate([[0], pat, [0]]).astype(np.int8)
    d = np.diff(e)
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1


def cuts_to_counts(cuts, total):
    cuts = sorted({int(c) for c in cuts if 0 < c < total})
    return np.diff([0] + cuts + [total]).astype(np.int32)


def count_sets(pat):
    total = pat.size
    rng = np.random.default_rng(20251)
    rand = []
    while sum(rand) < total:
        rand.append(min(int(rng.integers(1, 151)), total - sum(rand)))
    first, last = run_edges(pat)
    edges = np.concatenate([first, last])
    return {
        "ones": np.ones(total, dtype=np.int32),
        "whole": np.array([total], dtype=np.int32),
        "random": np.array(rand, dtype=np.int32),
        # a burst ends exactly at / one before / one after every run's first and last packet
        "at_edges": cuts_to_counts(edges, total),
        "before_edges": cuts_to_counts(edges - 1, total),
        "after_edges": cuts_to_counts(edges + 1, total),
    }


def check_pattern(T, B, N, pat):
    ref = fec.plan_host(L, T, B, N, pat)
    assert (ref == 2).any() and (ref == 3).any()  # recovered and lost packets are both exercised
    for name, counts in count_sets(pat).items():
        assert int(counts.sum()) == pat.size and (counts >= 1).all(), name
        got = fec.plan_burst_host(L, T, B, N, pat, counts)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (name, bad[:10].tolist())


@pytest.mark.parametrize("tbn", TUPLES)
def test_burst_planner_equals_plan_host_on_synthetic_pattern(tbn):
    T, B, N = tbn
    check_pattern(T, B, N, synthetic_pattern(T, B, N))


@pytest.mark.parametrize("tbn,pattern", [((10, 3, 3), "bin_erasure"), ((10, 5, 2), "erasure50")])
def test_burst_planner_equals_plan_host_on_shipped_patterns(tbn, pattern):
    T, B, N = tbn
    check_pattern(T, B, N, load_pattern(pattern)[:20000].astype(np.uint8))


def test_burst_planner_rejects_bad_counts():
    pat = np.zeros(40, dtype=np.uint8)
    for counts in ([40, 0], [41, -1]):
        with pytest.raises(fec.FecError):
            fec.plan_burst_host(L, 10, 3, 3, pat, np.array(counts, dtype=np.int32))
