"""Every instance of fec_recover_fast_kernel<k, n-k>, and of the copy kernels instantiated from the
same list, against the oracle.  Needs an MI355X: -m gpu.

The pairs are read from FEC_COPY_FAST_LIST (tests/test_recover_fast_host.py: 19 pairs, 18 of them
with parity), each mapped to its code (10, n-k, 11-k).  LMAX is the largest max_payload at which a
pair's staged span fits the 12 288-byte limit (derived from the span formula on the CPU there).  The
helpers and case bodies are those of tests/test_gpu_recover_fast.py; every expected byte, length
and count is the oracle's.

  every instance       L = 1 (S = 1, fewer items than lanes), 300 where the pair takes it, LMAX (the
                       span within 16 .. 244 bytes of the limit: the last staging chunk is live)
  each side of limit   LMAX + 1: "fast" refused, "auto" is the generic kernel
  (11, 0)              nothing to recover: every wave of the launch returns at once
  variable lengths     k = 1, lengths above 255, k * n = 150 (three coefficient registers per lane),
                       12 items for 64 lanes
  tiny batches         1, 2, k, n, n + 1 output rows at k = 1, 4 and 10, at LMAX
  unaligned buffers    (9, 3) at LMAX = 457: a span of 12 272 bytes moved across a 16-byte piece
  copy kernels         fec_copy_pair_kernel / fec_copy_fast_kernel of every pair at one L % 4 == 0
"""
import numpy as np
import pytest

import oracle
import test_gpu_recover_fast as rf
from test_gpu_buffers import Out, check_decode, garbled, place, refused
from test_recover_fast_host import LMAX, PAIRS, REC_PAIRS, tbn_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402

P_BASE = rf.P_BASE


def pair_id(v):
    return "k%d-np%d" % v if isinstance(v, tuple) else None


INSTANCE_CASES = [(pair, L) for pair in REC_PAIRS
                  for L in sorted({1, LMAX[pair]} | ({300} if LMAX[pair] >= 300 else set()))]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def test_the_sweep_holds_every_instance():
    assert len(PAIRS) == 19 and len(REC_PAIRS) == 18
    assert {p for p, _ in INSTANCE_CASES} == set(REC_PAIRS)
    for pair in REC_PAIRS:  # LMAX and one smaller size
        assert sum(1 for p, L in INSTANCE_CASES if p == pair and L < LMAX[pair]) >= 1
        assert (pair, LMAX[pair]) in INSTANCE_CASES


@pytest.mark.parametrize("pair,L", INSTANCE_CASES, ids=pair_id)
def test_every_instance(pair, L):
    k, np_ = pair
    tbn = tbn_of(pair)
    pat, ref = rf.base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    assert (c.k, c.n) == (k, k + np_)
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    rec = rf.decode_both(c, cw, er, ref["out_data"], ref["out_len"], P_BASE)
    assert c.info()["recover_kernel"].startswith(f"fec_recover_fast_kernel<{k}, {np_}>")  # the last path: fast
    assert rec == int(rf.recovered_rows(pat, ref["out_len"]).sum())


@pytest.mark.parametrize("pair", REC_PAIRS, ids=pair_id)
def test_past_the_staging_limit(pair):
    rf.refuse_fast_case(LMAX[pair] + 1, tbn_of(pair))


def test_nothing_to_recover():
    """(11, 0): no parity.  Every erased row is lost, and no wave of the recovery has a packet."""
    L, tbn = 300, tbn_of((11, 0))
    assert tbn == (10, 0, 0)
    pat, ref = rf.base_stream(L, tbn)
    erased = pat[:P_BASE] == 1
    assert (ref["out_len"][erased] == 0).all() and (ref["out_len"][~erased] > 0).all()
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    for path in ("generic", "fast") if rf.fast_applies(c) else ("generic",):
        rf.select(c, path)
        out, ln = Out((P_BASE, L)), Out((P_BASE,), dtype=torch.int32)
        c.decode(cw, er, out=out.t, out_len=ln.t)
        torch.cuda.synchronize()
        assert (ln.host() == ref["out_len"]).all(), path  # host(): the guards as well
        assert (out.host() == ref["out_data"]).all(), path
        eps, rec, lost = c.counters()
        assert rec == 0 and lost == int(erased.sum()) == 77, path


@pytest.mark.parametrize("L,tbn", [(99, (10, 10, 10)), (314, (10, 7, 7)), (338, (10, 5, 1)), (37, (10, 9, 8))])
def test_variable_lengths_at_the_extremes(L, tbn):
    rf.variable_lengths_case(L, tbn)


@pytest.mark.parametrize("L,tbn", [(99, (10, 10, 10)), (314, (10, 7, 7)), (338, (10, 5, 1))])
def test_tiny_batches_at_the_limit(L, tbn):
    row0 = rf.tiny_batches_case(L, tbn)
    pat, ref = rf.base_stream(L, tbn)
    if ref["out_len"][0] > 0:  # the oracle recovers an erased packet 0 with this code
        assert any(row0), "no size recovers row 0"


@pytest.mark.parametrize("cw_off", [1, 3])
@pytest.mark.parametrize("out_off", [0, 3])
def test_unaligned_buffers_at_the_limit(cw_off, out_off):
    pair = (9, 3)
    L, tbn = LMAX[pair], tbn_of(pair)
    assert (L, tbn) == (457, (10, 3, 2))
    k, n, S, CW = oracle.geometry(L, *tbn)
    assert (k + n - 1) * CW + 32 == 12272
    pat, ref = rf.base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(ref["cw"], pat, 7), cw_off), place(pat)
    rec = rf.decode_both(c, cw, er, ref["out_data"], ref["out_len"], P_BASE, out_off)
    assert rec >= rf.RECOVERED[tbn]


def copy_size(pair):
    if pair == (11, 0) or LMAX[pair] >= 300:
        return 300
    return LMAX[pair] & ~3


def round16(v):
    return (v + 15) & ~15


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_copy_kernels_of_every_pair(pair):
    """The LDS-tile copy exists where its smallest tile, 8 packets, fits 64 KB of LDS (codeword
    tile with 32 + 4n bytes of slack, payload tile, 5 bytes per packet, the T flags behind): there
    copy "fast" and "generic" both give the oracle's rows; elsewhere "fast" is refused."""
    k, np_ = pair
    L, tbn = copy_size(pair), tbn_of(pair)
    assert L % 4 == 0
    pat, ref = rf.base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    if round16(32 + 8 * c.CW + 4 * c.n) + round16(8 * L) + 5 * 8 + tbn[0] + 16 > 64 * 1024:
        refused(lambda: c.set_copy_path("fast"))
        return
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    for path in ("fast", "generic"):
        c.set_copy_path(path)
        name = c.info()["copy_kernel"]
        if path == "fast":
            assert name in (f"fec_copy_pair_kernel<{k}, {np_}>", f"fec_copy_fast_kernel<{k}, {np_}>"), name
        else:
            assert name == "fec_copy_kernel", name
        out, ln = Out((P_BASE, L)), Out((P_BASE,), dtype=torch.int32)
        c.decode(cw, er, out=out.t, out_len=ln.t)
        check_decode(c, out, ln, ref, pat, P_BASE, path)
