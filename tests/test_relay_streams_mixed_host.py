"""Mixed relay stream groups, the host-only half (fec_relay_streams_mixed_fit): per code the chunk of
a long burst and its LDS bytes on both sides, equal to the one-code fit of the same tuple, and which
lists of tuples a group refuses.  No GPU."""
import numpy as np
import pytest

from test_swdf import SWDF_CASES

import fec_erasure_code_unit_test_relay_amd as fec
from fec_erasure_code_unit_test_relay_amd.relay import relay_streams_fit, relay_streams_mixed_fit

LDS_PER_CU = 163840
ARG = fec._lib.FEC_ERR_ARG


@pytest.mark.parametrize("L", [300, 37])
def test_mixed_fit_equals_the_one_code_fit(L):
    rc, rl, dc, dl = relay_streams_mixed_fit(L, SWDF_CASES)
    for c, cfg in enumerate(SWDF_CASES):
        assert (True, int(rc[c]), int(rl[c])) == relay_streams_fit(True, L, *cfg), cfg
        assert (True, int(dc[c]), int(dl[c])) == relay_streams_fit(False, L, *cfg), cfg
        T1, N1, T2, N2 = cfg
        # a burst cut into several chunks takes the rows in front of a later chunk from the burst itself
        assert T1 + T2 <= rc[c] <= 32 and T2 <= dc[c] <= 32
        assert 0 < rl[c] <= LDS_PER_CU and 0 < dl[c] <= LDS_PER_CU
    if L == 300:
        # (10,10,10,10): k = 1, rows of 3 322 bytes; every other code runs the full chunk
        assert rc.tolist() == [32, 32, 32, 23, 32, 32]
        assert dc.tolist() == [32] * 6


def test_mixed_fit_at_mtu_payloads():
    two = [(10, 3, 10, 3), (10, 5, 8, 3)]
    rc, rl, dc, dl = relay_streams_mixed_fit(1500, two)
    assert rc.tolist() == [24, 19] and dc.tolist() == [32, 32]
    assert (rl > 65536).all() and (rl <= LDS_PER_CU).all() and (dl <= LDS_PER_CU).all()
    # (10,10,10,10) at L = 1500: 20 rows of 16 522 bytes in front of a packet exceed a CU's LDS
    assert relay_streams_fit(True, 1500, 10, 10, 10, 10) == (False, 0, 0)
    with pytest.raises(fec.FecError) as err:
        relay_streams_mixed_fit(1500, two + [(10, 10, 10, 10)])
    assert err.value.status == ARG


@pytest.mark.parametrize("tuples", [[], [(10, 3, 10, 3)] * 65, [(10, 3, 10, 3), (10, 3, 10, 4)]],
                         ids=["no-codes", "65-codes", "k-mismatch"])
def test_mixed_fit_rejects(tuples):
    with pytest.raises(fec.FecError) as err:
        relay_streams_mixed_fit(300, np.array(tuples, dtype=np.int32).reshape(-1, 4))
    assert err.value.status == ARG


def test_mixed_fit_accepts_64_codes_and_rejects_null_pointers():
    rc, _, dc, _ = relay_streams_mixed_fit(300, [(10, 3, 10, 3)] * 64)
    assert rc.tolist() == [32] * 64 and dc.tolist() == [32] * 64
    tup = np.array([(10, 3, 10, 3)], dtype=np.int32)
    a = np.zeros(1, dtype=np.int32)
    p = a.ctypes.data
    fit = fec.lib().fec_relay_streams_mixed_fit
    assert fit(300, None, 1, p, p, p, p) == ARG
    assert fit(300, tup.ctypes.data, 1, p, p, None, p) == ARG
    assert fit(300, tup.ctypes.data, 1, p, p, p, p) == 0
