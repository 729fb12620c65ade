"""CPU checks of the specialised recovery kernel's host-callable parts (fec_recover_fast.h through
fec_recover_fast_items / fec_recover_fast_mul): which geometries take it, that every source byte it
reads lies inside the codeword buffer, that every byte of [len_hi, len_lo, payload] is produced
exactly once, and all 65 536 products of the packed-doubling tables.  The kernel computes its
spans, item offsets and tables through the same functions.  No device work here.

The sweep covers every instance: the (k, n-k) pairs are read from FEC_COPY_FAST_LIST in
csrc/fec_kernels.h (19 of them; a new instance extends the sweep or fails it), the predicate is
compared with (k+n-1) * n * ceil((L+2)/k) + 32 <= 12 288 for every L up to 2000, the largest
payload size each pair accepts (LMAX) is derived from that formula, and the bounds and coverage are
checked for every pair at L = 1, 2, 300 (where it applies) and LMAX.  tests/test_gpu_recover_fast.py
takes the pairs and LMAX from here."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle

import fec_erasure_code_unit_test_relay_amd as fec

STAGE_MAX = 12 * 1024  # kRecFastStageMax (fec_recover_fast.h)

# (max_payload, (T, B, N)): the seven sizes of tests/test_gpu_recover_fast.py and (10,10,10);
# every_pair_sizes() below adds each instance's
SIZES = [(300, (10, 3, 3)), (300, (10, 5, 2)), (300, (10, 1, 1)), (64, (10, 5, 2)), (2, (10, 3, 3)),
         (301, (10, 3, 3)), (299, (10, 4, 3)), (300, (10, 10, 10))]

# work items per packet k * ceil(S / 4) where the kernel applies, 0 where it does not: no instance
# for (k, n-k), or the k+n-1 rows of CW bytes (+ 32) exceed the 12 KB staging limit
APPLIES = {
    (300, (10, 3, 3)): 8 * 10,    # k 8, n 11, S 38, CW 418: 18 rows, 7 556 bytes
    (300, (10, 5, 2)): 9 * 9,     # k 9, n 14, S 34, CW 476: 22 rows, 10 504 bytes
    (300, (10, 1, 1)): 10 * 8,    # k 10, n 11, S 31, CW 341
    (64, (10, 5, 2)): 9 * 2,      # S 8
    (2, (10, 3, 3)): 8 * 1,       # S 1
    (301, (10, 3, 3)): 8 * 10,
    (299, (10, 4, 3)): 8 * 10,    # k 8, n 12, S 38
    (300, (10, 10, 10)): 0,       # k 1, n 11, CW 3 322: 11 rows, 36 574 bytes
    (1500, (10, 3, 3)): 0,        # CW 2 068: 18 rows, 37 256 bytes
    (300, (10, 9, 8)): 0,         # k 3, n 12, CW 1 212: 14 rows, 17 000 bytes
    (300, (10, 9, 9)): 0,         # k 2, n 11, CW 1 661
    (300, (10, 9, 1)): 0,         # n 19: no instance
    (300, (10, 8, 4)): 0,         # (7, 8): no instance
    (300, (10, 4, 4)): 7 * 11,    # k 7, n 11, S 44, CW 484: 17 rows, 8 260 bytes
    (37, (10, 9, 8)): 3 * 4,      # k 3, n 12, S 13, CW 156
}

# Largest max_payload at which fec_recover_fast_kernel<k, n-k> applies, per (k, n-k): the staged span
# (k+n-1) * n * ceil((L+2)/k) + 32 is then the closest to the 12 288-byte limit.  Derived again from
# the formula in test_predicate_equals_formula.
LMAX = {(8, 3): 486, (9, 5): 349, (10, 1): 548, (9, 2): 520, (7, 4): 453, (6, 5): 412, (5, 6): 368,
        (4, 7): 314, (3, 8): 253, (2, 9): 182, (1, 10): 99, (10, 3): 418, (9, 3): 457, (10, 4): 378,
        (8, 4): 422, (10, 5): 338, (7, 5): 390, (3, 9): 214}


def fast_pairs():
    """The (k, n-k) pairs of FEC_COPY_FAST_LIST, in the header's order."""
    path = os.path.join(os.path.dirname(os.path.abspath(fec.__file__)), "csrc", "fec_kernels.h")
    with open(path) as f:
        text = f.read()
    body = re.search(r"#define\s+FEC_COPY_FAST_LIST\(X\)((?:[^\n]*\\\n)*[^\n]*)", text).group(1)
    return [(int(k), int(np_)) for k, np_ in re.findall(r"\bX\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]


PAIRS = fast_pairs()
REC_PAIRS = [p for p in PAIRS if p[1] > 0]  # (11, 0) recovers nothing


def tbn_of(pair):
    """(k, n-k) -> (T, B, N) at T = 10: k = T - N + 1, n = k + B."""
    k, np_ = pair
    return (10, np_, 11 - k)


def span_formula(k, n, L):
    """Bytes of the widest staged span: k+n-1 codeword rows of n * ceil((L+2)/k) bytes, + 32."""
    return (k + n - 1) * n * (-(-(L + 2) // k)) + 32


def every_pair_sizes():
    """Each instance at L = 1, 2, 300 (where it applies) and its LMAX, with the work items per packet
    k * ceil(S / 4) computed here for the sizes APPLIES does not list."""
    sizes = []
    for k, np_ in REC_PAIRS:
        lmax = LMAX[(k, np_)]
        for L in sorted({1, 2, lmax} | ({300} if lmax >= 300 else set())):
            key = (L, tbn_of((k, np_)))
            S = -(-(L + 2) // k)
            APPLIES.setdefault(key, k * (-(-S // 4)))
            if key not in SIZES and key not in sizes:
                sizes.append(key)
    return sizes


SIZES = SIZES + every_pair_sizes()


def items(L, tbn, P=0, x=0, span=None, src=None, out=None):
    vp = ctypes.c_void_p
    return fec.lib().fec_recover_fast_items(L, *tbn, P, x, span.ctypes.data_as(vp) if span is not None else None,
                                            src.ctypes.data_as(vp) if src is not None else None,
                                            out.ctypes.data_as(vp) if out is not None else None)


def test_predicate_table():
    for (L, tbn), want in APPLIES.items():
        assert items(L, tbn) == want, (L, tbn)
    assert items(300, (10, 1, 3)) == -1  # B < N
    assert set(SIZES) <= set(APPLIES)


def test_pair_list():
    """19 distinct instances; each maps to a code (10, B, N) with B >= N, but for (11, 0)."""
    assert len(PAIRS) == 19 and len(set(PAIRS)) == 19, PAIRS
    assert set(REC_PAIRS) == set(LMAX) and len(REC_PAIRS) == 18
    assert set(PAIRS) - set(REC_PAIRS) == {(11, 0)}
    for pair in PAIRS:
        k, np_ = pair
        T, B, N = tbn_of(pair)
        assert (T - N + 1, T - N + 1 + B) == (k, k + np_) and 0 <= N <= T
        assert B >= N or pair == (11, 0), pair
    assert tbn_of((11, 0)) == (10, 0, 0)
    assert items(300, (10, 0, 0)) == -1  # N = 0: nothing to recover, rejected
    # the sweep of test_bounds_and_coverage holds every instance at its smallest and largest size
    for pair in REC_PAIRS:
        assert {(1, tbn_of(pair)), (LMAX[pair], tbn_of(pair))} <= set(SIZES), pair


@pytest.mark.parametrize("pair", REC_PAIRS, ids=lambda p: "k%d-np%d" % p)
def test_predicate_equals_formula(pair):
    """fec_recover_fast_items > 0 exactly where the span formula fits the staging limit, for every
    L in 1 .. 2000; the largest such L is the table's LMAX and its item count k * ceil(S / 4)."""
    k, np_ = pair
    n = k + np_
    tbn = tbn_of(pair)
    fits = []
    for L in range(1, 2001):
        want = span_formula(k, n, L) <= STAGE_MAX
        got = items(L, tbn)
        assert (got > 0) == want, (pair, L, got)
        if want:
            S = -(-(L + 2) // k)
            assert got == k * (-(-S // 4)), (pair, L, got)
            fits.append(L)
        else:
            assert got == 0, (pair, L, got)
    lmax = max(fits)
    assert fits == list(range(1, lmax + 1))  # the span grows with L
    assert lmax == LMAX[pair], (pair, lmax)
    assert span_formula(k, n, lmax) <= STAGE_MAX < span_formula(k, n, lmax + 1)


@pytest.mark.parametrize("L,tbn", SIZES)
def test_bounds_and_coverage(L, tbn):
    T, B, N = tbn
    k = T - N + 1
    n = k + B
    S = -(-(L + 2) // k)
    CW = S * n
    nit = items(L, tbn)
    assert nit == APPLIES[(L, tbn)]
    if nit == 0:
        return
    it = np.arange(nit)
    g, i = it // k, it % k
    q = np.arange(n)
    e = np.arange(4)
    span = np.zeros(5, dtype=np.int64)
    src = np.zeros((nit, n, 4), dtype=np.int64)
    out = np.zeros((nit, 4), dtype=np.int32)
    sub = 4 * g[:, None, None] + e[None, None, :]                        # sub-stream of (item, e)
    want_out = np.where((sub[:, 0, :] < S) & (sub[:, 0, :] * k + i[:, None] < L + 2),
                        sub[:, 0, :] * k + i[:, None], -1)
    for P in list(range(1, 41)) + [600]:
        Pout = P - T
        if Pout <= 0:
            assert items(L, tbn, P, 0, span) == -1  # no output row
            continue
        for x in range(Pout):
            assert items(L, tbn, P, x, span, src, out) == nit
            rlo, rhi, b0, b1, lds = (int(v) for v in span)
            assert (rlo, rhi) == (max(0, x - k + 1), min(P, x + n))
            assert 0 <= b0 <= rlo * CW and rhi * CW <= b1 <= P * CW, (P, x)  # the staged bytes: in the buffer
            assert b0 % 16 == 0 and b1 - b0 <= lds <= 12 * 1024
            # term q of item (i, g), sub-stream e: byte (4g+e) * n + q of row x-i+q, or absent
            row = x - i[:, None, None] + q[None, :, None]
            present = (row >= 0) & (row < P) & (sub < S)
            want = np.where(present, row * CW + sub * n + q[None, :, None], -1)
            assert (src == want).all(), (P, x)
            got = src[src >= 0]
            assert got.size == 0 or (got.min() >= b0 and got.max() < b1)  # inside what the wave staged
            assert got.size == 0 or (got.min() >= 0 and got.max() < P * CW)
            if x >= k - 1 and x + n <= P:
                assert present[sub.repeat(n, axis=1) < S].all()
            # every byte of [len_hi, len_lo, payload] exactly once, nothing past L + 2
            assert (out == want_out).all()
            assert (np.sort(out[out >= 0]) == np.arange(L + 2)).all(), (P, x)
            pay = out[out >= 2].astype(np.int64) - 2
            assert pay.min() >= 0 and pay.max() < L
            for row_off in range(4):  # a continuing decode: packet x goes to row x - row_off, or is skipped
                if x >= row_off:
                    at = (x - row_off) * L + pay
                    assert at.min() >= 0 and at.max() < (Pout - row_off) * L


def test_packed_product_all_pairs():
    """c * x for all 65 536 pairs: the tables gf_mul4x_tables builds by packed doubling, read as the
    kernel's gf_mul4x reads them, against the oracle's gf_mul."""
    x = np.arange(256, dtype=np.uint32).reshape(64, 4)
    words = (x[:, 0] | (x[:, 1] << 8) | (x[:, 2] << 16) | (x[:, 3] << 24)).astype(np.uint32)
    mul = fec.lib().fec_recover_fast_mul
    for c in range(256):
        got = np.array([mul(c, int(w)) for w in words], dtype=np.uint32)
        got = np.stack([(got >> (8 * b)) & 0xff for b in range(4)], axis=1).reshape(256)
        want = np.array([oracle.gf_mul(c, v) for v in range(256)], dtype=np.uint32)
        assert (got == want).all(), c
