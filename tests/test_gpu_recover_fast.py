"""The (k, n-k)-specialised recovery kernel (fec_recover_fast.hip) against the oracle, beside the
generic one on the same inputs.  Needs an MI355X: -m gpu.

Every case decodes with set_recover_path("generic") and with "fast"; both must equal the oracle bit
for bit.  Where info() says the specialised kernel applies, "fast" is selected and info() must then
name it (a codec or call it does not apply to is refused with FEC_ERR_ARG, never served by the other
kernel); every case also asserts, from the oracle alone, that its pattern recovers packets.

The packed product is checked for all 65 536 pairs on the CPU (tests/test_recover_fast_host.py: the
table builder is host-callable), so no crafted stream is needed for it here.  No decode test of
this suite runs under graph capture, so there is none here either.

The cases of this file stay around four (k, n-k) pairs; tests/test_gpu_recover_fast_pairs.py runs
every instance of FEC_COPY_FAST_LIST through the helpers and case bodies defined here (RECOVERED
and NO_EDGE_ROWS hold the oracle's figures for every code of that sweep)."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_buffers import Out, garbled, place

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402
from fec_erasure_code_unit_test_relay_amd._lib import FEC_ERR_ARG  # noqa: E402

SEED = 0x5EED
P_BASE = 600
FAST_SIZES = [(300, (10, 3, 3)), (300, (10, 5, 2)), (300, (10, 1, 1)), (64, (10, 5, 2)), (2, (10, 3, 3)),
              (301, (10, 3, 3)), (299, (10, 4, 3))]
GENERIC_SIZES = [(300, (10, 10, 10)), (300, (10, 9, 1))]  # long codewords; n = 19 (tests/test_gpu_parity.py DEC_CASES)
# recovered packets of the base pattern on the CPU oracle, per (T, B, N)
RECOVERED = {(10, 3, 3): 43, (10, 5, 2): 43, (10, 4, 3): 43, (10, 1, 1): 37, (10, 10, 10): 57, (10, 9, 1): 44,
             # the other codes of FEC_COPY_FAST_LIST: the same count at L = 1, 300, the largest L
             # the specialised kernel takes and that L + 1
             (10, 2, 2): 37, (10, 4, 4): 47, (10, 5, 5): 47, (10, 6, 6): 49, (10, 7, 7): 51, (10, 8, 8): 53,
             (10, 9, 9): 55, (10, 3, 1): 38, (10, 3, 2): 41, (10, 4, 1): 42, (10, 5, 1): 42, (10, 5, 4): 47,
             (10, 9, 8): 54, (10, 0, 0): 0}
# codes whose oracle does not recover all of rows 0, 1, 3, P-3 and P-1 of the base pattern
NO_EDGE_ROWS = {(10, 1, 1), (10, 2, 2), (10, 3, 1), (10, 3, 2), (10, 4, 1), (10, 5, 1), (10, 0, 0)}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def base_pattern(P, T):
    """Erased rows in front of the stream (their diagonals start before packet 0) and at its end,
    isolated erasures, a burst that is recovered and one that is lost."""
    pat = np.zeros(P + T, dtype=np.uint8)
    pat[[0, 1, 3]] = 1
    pat[40:P - 20:13] = 1
    pat[200:203] = 1
    pat[300:330] = 1
    pat[P - 3] = pat[P - 1] = 1
    pat[P + 2] = 1
    return pat


def recovered_rows(pat, out_len):
    return (pat[:out_len.size] == 1) & (out_len > 0)


@functools.lru_cache(maxsize=None)
def base_stream(L, tbn):
    """The base pattern's stream at (L, tbn) through the oracle, once per module (the tests only read it)."""
    T = tbn[0]
    pat = base_pattern(P_BASE, T)
    ref = oracle.run_stream(L, *tbn, P_BASE, pat, seed=SEED, want_data=True, want_codewords=True)
    rec = recovered_rows(pat, ref["out_len"])
    assert int(pat[:P_BASE].sum()) == 77
    assert int(rec.sum()) >= RECOVERED[tbn], (L, tbn, int(rec.sum()))
    if tbn not in NO_EDGE_ROWS:
        assert rec[[0, 1, 3, P_BASE - 3, P_BASE - 1]].all()
    return pat, ref


def fast_applies(c):
    c.set_recover_path("auto")
    return c.info()["recover_kernel"].startswith("fec_recover_fast_kernel")


def select(c, path):
    """Select `path`; "fast" must then be the kernel info() names."""
    c.set_recover_path(path)
    name = c.info()["recover_kernel"]
    if path == "fast":
        assert name.startswith(f"fec_recover_fast_kernel<{c.k}, {c.n - c.k}>"), name
    else:
        assert name.startswith("fec_recover_kernel_t<"), name


def decode_both(c, cw, er, want, want_len, P, out_off=0):
    """The decode of `cw` on both recovery paths, each into fresh guarded buffers."""
    assert fast_applies(c)
    for path in ("generic", "fast"):
        select(c, path)
        out, ln = Out((P, c.L), out_off), Out((P,), dtype=torch.int32)
        c.decode(cw, er, out=out.t, out_len=ln.t)
        torch.cuda.synchronize()
        assert (ln.host() == want_len).all(), path
        assert (out.host() == want).all(), path
    return c.counters()[1]


@pytest.mark.parametrize("L,tbn", FAST_SIZES)
def test_fast_sizes(L, tbn):
    pat, ref = base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    rec = decode_both(c, cw, er, ref["out_data"], ref["out_len"], P_BASE)
    assert rec == int(recovered_rows(pat, ref["out_len"]).sum())
    info = c.info()
    assert info["recover_waves"] == 4096 and info["recover_wave_rows"] == 16


@pytest.mark.parametrize("L,tbn", GENERIC_SIZES)
def test_generic_sizes_refuse_fast(L, tbn):
    refuse_fast_case(L, tbn)


def refuse_fast_case(L, tbn):
    """A size the specialised kernel does not take: "fast" refused, "auto" and "generic" the oracle's."""
    pat, ref = base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    assert not fast_applies(c)
    with pytest.raises(fec.FecError) as e:
        c.set_recover_path("fast")
    assert e.value.status == FEC_ERR_ARG
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    for path in ("auto", "generic"):
        select(c, path)
        out, ln = Out((P_BASE, L)), Out((P_BASE,), dtype=torch.int32)
        c.decode(cw, er, out=out.t, out_len=ln.t)
        assert (ln.host() == ref["out_len"]).all(), path
        assert (out.host() == ref["out_data"]).all(), path


@pytest.mark.parametrize("L,tbn", [(300, (10, 3, 3)), (301, (10, 3, 3)), (64, (10, 5, 2))])
def test_variable_lengths(L, tbn):
    variable_lengths_case(L, tbn)


def variable_lengths_case(L, tbn):
    """Recovered rows of length 0, of length L and in between: zero tail and length word, against the
    oracle's per-packet coders."""
    pat, cws, want, want_len = variable_lengths_ref(L, tbn)
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(cws, pat, L)), place(pat)
    decode_both(c, cw, er, want, want_len, P_BASE)


def variable_lengths_ref(L, tbn):
    """The oracle's half of variable_lengths_case (no device): pattern, codewords, rows, lengths."""
    T, B, N = tbn
    rows = P_BASE + T
    pat = base_pattern(P_BASE, T)
    lens = np.random.default_rng(L).integers(0, L + 1, size=rows).astype(np.int32)
    lens[::9] = L
    lens[1], lens[3], lens[40] = 0, L // 3, 1  # row 0 is a ninth row: L
    src = oracle.fill_payload(0, rows, L, 5)
    enc, dec = oracle.Encoder(L, T, B, N), oracle.Decoder(L, T, B, N)
    cws, want, want_len = [], [], []
    for t in range(rows):
        cw, size = enc.onTransmit(src[t], int(lens[t]), t)
        cws.append(cw)
        o, p = dec.onReceive(None if pat[t] else cw, size, t, bool(pat[t]))
        if t >= T:
            want.append(o)
            want_len.append(p)
    want, want_len = np.stack(want), np.array(want_len)
    rec = recovered_rows(pat, want_len)
    # (a recovered row of length 0 reads as lost here)
    assert int(rec.sum()) >= RECOVERED[tbn] - int(((pat[:P_BASE] == 1) & (lens[:P_BASE] == 0)).sum())
    assert want_len[0] == L and want_len[3] == L // 3 and want_len[40] == 1 and (want[1] == 0).all()
    return pat, np.stack(cws), want, want_len


def test_tiny_batches():
    """1, 2, k, n and n + 1 output rows, packet 0 erased: what is recovered is the oracle's to say."""
    assert any(tiny_batches_case(300, (10, 3, 3))), "no size recovers row 0"


def tiny_batches_case(L, tbn):
    """The loop of test_tiny_batches; per size, whether the oracle recovers row 0."""
    T = tbn[0]
    c = fec.Codec(L, *tbn)
    row0 = []
    for P in dict.fromkeys((1, 2, c.k, c.n, c.n + 1)):
        pat = np.zeros(P + T, dtype=np.uint8)
        pat[0] = 1
        ref = oracle.run_stream(L, *tbn, P, pat, seed=SEED + P, want_data=True, want_codewords=True)
        row0.append(bool(ref["out_len"][0] > 0))
        cw, er = place(garbled(ref["cw"], pat, P)), place(pat)
        decode_both(c, cw, er, ref["out_data"], ref["out_len"], P)
    return row0


@pytest.mark.parametrize("cw_off,out_off", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2), (3, 3)])
def test_unaligned_buffers(cw_off, out_off):
    L, tbn = 300, (10, 3, 3)
    pat, ref = base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(ref["cw"], pat, 7), cw_off), place(pat)
    rec = decode_both(c, cw, er, ref["out_data"], ref["out_len"], P_BASE, out_off)
    assert rec >= RECOVERED[tbn]


def test_more_recovered_packets_than_waves():
    """Isolated erasures every 12th packet against a launch of one wave per 16 output rows: the
    waves walk the list (r += waves)."""
    L, tbn, P = 300, (10, 3, 3), 6000
    T = tbn[0]
    pat = np.zeros(P + T, dtype=np.uint8)
    pat[5::12] = 1
    ref = oracle.run_stream(L, *tbn, P, pat, seed=SEED, want_data=True, want_codewords=True)
    c = fec.Codec(L, *tbn)
    assert fast_applies(c)
    select(c, "fast")
    info = c.info()
    waves = min(info["recover_waves"], -(-P // info["recover_wave_rows"]))
    nrec = int(recovered_rows(pat, ref["out_len"]).sum())
    assert nrec >= 1.25 * waves, (nrec, waves)
    cw, er = place(garbled(ref["cw"], pat, 3)), place(pat)
    assert decode_both(c, cw, er, ref["out_data"], ref["out_len"], P) == nrec


def test_continuing_decode():
    """DecodeStream.push in three chunks, the second and third restarting in front of their first
    output row (row_off > 0: the cuts fall in the lost burst), against the one-shot decode."""
    L, tbn = 300, (10, 3, 3)
    T = tbn[0]
    pat, ref = base_stream(L, tbn)
    c = fec.Codec(L, *tbn)
    assert fast_applies(c)
    cw, er = place(garbled(ref["cw"], pat, 11)), place(pat)
    for path in ("generic", "fast"):
        select(c, path)
        ds = fec.DecodeStream(c)
        outs, lens, a, offs = [], [], 0, []
        for b in (315, 450, P_BASE + T):
            out, ln = Out((b - a, L)), Out((b - a,), dtype=torch.int32)
            o, n = ds.push(cw[:b], er[:b], pat[:b], history=a, out=out.t, out_len=ln.t)
            torch.cuda.synchronize()
            out.check()
            ln.check()
            outs.append(o.cpu().numpy())
            lens.append(n.cpu().numpy())
            offs.append(max(0, a - T) - ds.state()[1])
            a = b
        assert offs[0] == 0 and offs[1] > 0, offs
        assert (np.concatenate(lens) == ref["out_len"]).all(), path
        assert (np.concatenate(outs) == ref["out_data"]).all(), path
