"""Mixed message-wise relay groups, the host-only half (fec_mw_relay_streams_mixed_fit): per pair the
chunk of a burst cut in several and its LDS bytes, equal to the one-code fit of the same pair, and which
lists of pairs a group refuses.  No GPU."""
import numpy as np
import pytest

from test_gpu_mw_relay_streams import PAIRS

import fec_erasure_code_unit_test_relay_amd as fec
from fec_erasure_code_unit_test_relay_amd.relay import mw_relay_streams_fit, mw_relay_streams_mixed_fit

ARG = fec._lib.FEC_ERR_ARG
MTU_PAIRS = [((10, 3, 3), (10, 3, 3)), ((10, 5, 2), (6, 2, 2))]


def front(pair):
    """The packets a later chunk of a cut burst needs in front of it: T1+k1-1 + n2-1."""
    (T1, _, N1), (T2, B2, N2) = pair
    k1, n2 = T1 - N1 + 1, T2 - N2 + 1 + B2
    return T1 + k1 - 1 + n2 - 1


@pytest.mark.parametrize("L", [300, 37])
def test_mixed_fit_equals_the_one_code_fit(L):
    chunk, lds = mw_relay_streams_mixed_fit(L, PAIRS)
    assert chunk.dtype == np.int32 and lds.dtype == np.int32 and chunk.shape == lds.shape == (len(PAIRS),)
    for c, pair in enumerate(PAIRS):
        assert (int(chunk[c]), int(lds[c])) == mw_relay_streams_fit(L, *pair), pair
        assert front(pair) <= chunk[c] <= 32 and 0 < lds[c] <= 160 * 1024


def test_mixed_fit_at_mtu_payloads():
    chunk, lds = mw_relay_streams_mixed_fit(1500, MTU_PAIRS)
    for c, pair in enumerate(MTU_PAIRS):
        assert (int(chunk[c]), int(lds[c])) == mw_relay_streams_fit(1500, *pair), pair
        assert front(pair) <= chunk[c] < 32
        assert 64 * 1024 < lds[c] <= 160 * 1024
    assert chunk[0] != chunk[1]  # two chunk sizes in one launch


@pytest.mark.parametrize("L,pairs", [(300, PAIRS[:2] + [((10, 2, 3), (10, 3, 3))]),     # B1 < N1
                                     (1500, MTU_PAIRS + [((24, 12, 12), (24, 12, 12))]),  # no chunk fits a CU
                                     (300, []), (300, [PAIRS[0]] * 65)],
                         ids=["B1<N1", "too-large-at-mtu", "no-pairs", "65-pairs"])
def test_mixed_fit_rejects(L, pairs):
    with pytest.raises(fec.FecError) as err:
        mw_relay_streams_mixed_fit(L, np.array(pairs, dtype=np.int32).reshape(-1, 6))
    assert err.value.status == ARG


def test_mixed_fit_accepts_64_pairs_and_rejects_null_pointers():
    chunk, lds = mw_relay_streams_mixed_fit(300, [PAIRS[1]] * 64)
    assert chunk.tolist() == [mw_relay_streams_fit(300, *PAIRS[1])[0]] * 64 and len(set(lds.tolist())) == 1
    pr = np.array([PAIRS[0]], dtype=np.int32).reshape(-1, 6)
    a = np.zeros(1, dtype=np.int32)
    p = a.ctypes.data
    fit = fec.lib().fec_mw_relay_streams_mixed_fit
    assert fit(300, None, 1, p, p) == ARG
    assert fit(300, pr.ctypes.data, 1, None, p) == ARG
    assert fit(300, pr.ctypes.data, 1, p, None) == ARG
    assert fit(300, pr.ctypes.data, 1, p, p) == 0
