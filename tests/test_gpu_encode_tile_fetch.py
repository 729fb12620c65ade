"""The tile encoder fetches only the payload rows a tile needs (fec_encode_tile.hip): the pieces of
its LDS-DMA past the tile's R rows are issued out of range.  Codewords and wire sizes against the
oracle around every tile boundary, with every length of history, the payload rows lying inside a
larger buffer of 0xA5 bytes that no codeword may show.  Needs an MI355X: -m gpu.

The encoder is causal, so oracle.encode_stream(L, T, B, N, 0, h + P) is the first h + P rows of
one longer stream: the reference of a tuple is computed once, for the longest case, and sliced."""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402
from fec_erasure_code_unit_test_relay_amd._lib import lib  # noqa: E402

L = 300
SEED = 29
GUARD = 64  # rows of 0xA5 in front of row -h and behind row P-1
TUPLES = {(10, 3, 3): 24, (10, 5, 2): 28, (10, 1, 1): 32, (10, 0, 0): 36, (10, 6, 6): 16}  # (T,B,N): R
P_MAX = 70001  # three tiles per workgroup


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def surrounded(rows: "torch.Tensor"):
    """rows copied into the middle of a larger device buffer filled with 0xA5; the view of them."""
    buf = torch.full((rows.shape[0] + 2 * GUARD,) + tuple(rows.shape[1:]), 0xA5 if rows.dtype == torch.uint8 else
                     0x25A5A5A5, dtype=rows.dtype, device="cuda")
    buf[GUARD:GUARD + rows.shape[0]] = rows
    return buf[GUARD:GUARD + rows.shape[0]]


def tile_codec(tbn):
    c = fec.Codec(L, *tbn)
    c.set_encode_path("tile")  # raises where no tile kernel exists: every tuple here has one
    return c


@pytest.mark.parametrize("tbn", list(TUPLES))
def test_tile_boundaries_and_history(tbn):
    T, B, N = tbn
    R, n = TUPLES[tbn], T - N + 1 + B
    geo = [ctypes.c_int() for _ in range(4)]
    assert lib().fec_encode_tile_fetch(L, T, B, N, 0, *map(ctypes.byref, geo)) == 1 and geo[0].value == R
    c = tile_codec(tbn)
    hs = sorted({0, 1, max(n - 2, 0), n - 1})
    ref = oracle.encode_stream(L, T, B, N, 0, max(hs) + P_MAX, seed=SEED)
    payload = fec.fill_payload(0, max(hs) + P_MAX, L, SEED)
    for P in (1, R - 1, R, R + 1, 2 * R + 1, P_MAX):
        for h in hs:
            rows = surrounded(payload[:h + P])
            cw, wl = c.encode(rows, history=h)
            assert (cw.cpu().numpy() == ref["cw"][h:h + P]).all(), (tbn, P, h)
            assert (wl.cpu().numpy() == ref["cw_len"][h:h + P]).all(), (tbn, P, h)


def test_variable_lengths_in_garbage_surround():
    """(10,3,3) with a length array holding 0 and 1 (as test_encode_variable_lengths_and_history),
    payload rows and lengths both inside a larger buffer of garbage."""
    T, B, N = 10, 3, 3
    P = 700
    rng = np.random.default_rng(3)
    lens = rng.integers(0, L + 1, size=P).astype(np.int32)
    lens[::7] = 0
    lens[1::11] = 1
    payload = fec.fill_payload(0, P, L, 9)
    enc = oracle.Encoder(L, T, B, N)
    host = payload.cpu().numpy()
    ref = np.stack([enc.onTransmit(host[t], int(lens[t]), t)[0] for t in range(P)])
    c = tile_codec((T, B, N))
    dl = torch.from_numpy(lens).cuda()
    cw, _ = c.encode(surrounded(payload), surrounded(dl))
    assert (cw.cpu().numpy() == ref).all()
    # the stream's tail as a batch of its own behind the full n-1 = 10 packets of history
    for cut in (24, 25, 49, 400):
        cw2, _ = c.encode(surrounded(payload[cut - 10:]), surrounded(dl[cut - 10:]), history=10)
        assert (cw2.cpu().numpy() == ref[cut:]).all(), cut
    # shorter histories: the rows in front of them count as never sent, so the reference is a
    # fresh encoder started at row s
    for h, s in [(0, 23), (1, 47), (9, 16)]:
        enc = oracle.Encoder(L, T, B, N)
        ref2 = np.stack([enc.onTransmit(host[t], int(lens[t]), t - s)[0] for t in range(s, P)])
        cw3, _ = c.encode(surrounded(payload[s:]), surrounded(dl[s:]), history=h)
        assert (cw3.cpu().numpy() == ref2[h:]).all(), (h, s)
