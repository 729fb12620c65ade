"""CPU checks of the message-wise relay group's chunk geometry (fec_mw_relay_streams_fit), through the
routine create and the relay call use: a chunk of a burst cut in several holds at least the
T1+k1-1 hop-1 codewords and the n2-1 messages a later chunk needs in front of it, at most 32 packets,
within a CU's 160 KB of LDS.  No device work here."""
import pytest

import fec_erasure_code_unit_test_relay_amd as fec
from fec_erasure_code_unit_test_relay_amd.relay import mw_relay_streams_fit

LDS = 160 * 1024


def front(code1, code2):
    (T1, _, N1), (T2, B2, N2) = code1, code2
    k1 = T1 - N1 + 1
    n2 = T2 - N2 + 1 + B2
    return T1 + k1 + n2 - 2


def test_fit_geometry():
    lds = {}
    for L, code1, code2 in [(300, (10, 3, 3), (10, 3, 3)), (300, (10, 5, 2), (6, 2, 2)),
                            (1500, (10, 3, 3), (10, 3, 3))]:
        chunk, nbytes = mw_relay_streams_fit(L, code1, code2)
        assert front(code1, code2) <= chunk <= 32, (L, code1, code2, chunk)
        assert 0 < nbytes <= LDS, (L, code1, code2, nbytes)
        lds[(L, code1, code2)] = nbytes
    assert lds[(1500, (10, 3, 3), (10, 3, 3))] >= lds[(300, (10, 3, 3), (10, 3, 3))]


def test_fit_refusals():
    for L, code1, code2 in [(300, (10, 2, 3), (10, 3, 3)),         # B1 < N1: fec_streams_create refuses it
                            (300, (10, 3, 3), (10, 2, 3)),         # B2 < N2
                            (1500, (24, 12, 12), (24, 12, 12))]:   # the smallest chunk (36 + 24 packets) cannot fit
        with pytest.raises(fec.FecError) as e:
            mw_relay_streams_fit(L, code1, code2)
        assert e.value.status == fec._lib.FEC_ERR_ARG, (L, code1, code2)
