"""CPU checks of a mixed stream group's chunk sizing (fec_streams_mixed_fit): per code the packets
per chunk and the LDS bytes of the encode and decode chunks, through the routines the calls use.  A
chunk holds at least the packets it needs in front of it (n-1 windows / T+k-1 codewords), at most
32, and fits a CU's 160 KB of LDS; a code's figures do not depend on the other codes of the group.
No device work here."""
import ctypes

import numpy as np
import pytest

import fec_erasure_code_unit_test_relay_amd as fec

SIX = [(10, 3, 3), (10, 5, 2), (10, 1, 1), (10, 0, 0), (3, 2, 2), (4, 4, 4)]
LDS = 160 * 1024


def fronts(T, B, N):
    k = T - N + 1
    return k + B - 1, T + k - 1


def test_six_codes_fit_at_300_bytes():
    ec, el, dc, dl = fec.streams_mixed_fit(300, SIX)
    for c, (T, B, N) in enumerate(SIX):
        fe, fd = fronts(T, B, N)
        assert max(1, fe) <= ec[c] <= 32, (T, B, N, ec[c])
        assert max(1, fd) <= dc[c] <= 32, (T, B, N, dc[c])
        assert 0 < el[c] <= LDS and 0 < dl[c] <= LDS, (T, B, N, el[c], dl[c])


def test_a_codes_figures_do_not_depend_on_the_group():
    among = fec.streams_mixed_fit(300, SIX)
    for c, tbn in enumerate(SIX):
        alone = fec.streams_mixed_fit(300, [tbn])
        assert [int(a[0]) for a in alone] == [int(a[c]) for a in among], tbn


def test_mtu_payloads_take_more_than_64_kb_and_the_widest_code_does_not_fit():
    two = [(10, 3, 3), (10, 5, 2)]
    ec, el, dc, dl = fec.streams_mixed_fit(1500, two)
    for c, (T, B, N) in enumerate(two):
        fe, fd = fronts(T, B, N)
        assert fe <= ec[c] <= 32 and fd <= dc[c] <= 32
        assert 65536 < el[c] <= LDS and 65536 < dl[c] <= LDS
    with pytest.raises(fec.FecError) as e:
        fec.streams_mixed_fit(1500, two + [(24, 12, 12)])
    assert e.value.status == fec._lib.FEC_ERR_ARG


def test_bad_arguments():
    for tuples in ([], [(10, 3, 3)] * 65, None, [(10, 3, 3), (3, 2, 4)]):  # 0 codes, 65, null, N > T
        with pytest.raises(fec.FecError) as e:
            fec.streams_mixed_fit(300, tuples)
        assert e.value.status == fec._lib.FEC_ERR_ARG
    # a null result pointer
    tup = np.array([(10, 3, 3)], dtype=np.int32)
    res = np.zeros(1, dtype=np.int32)
    p = res.ctypes.data_as(ctypes.c_void_p)
    st = fec.lib().fec_streams_mixed_fit(300, tup.ctypes.data_as(ctypes.c_void_p), 1, p, p, None, p)
    assert st == fec._lib.FEC_ERR_ARG
    assert len(fec.streams_mixed_fit(300, [(10, 3, 3)] * 64)[0]) == 64
