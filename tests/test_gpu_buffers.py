"""The batched kernels at payload sizes that are not whole dwords and at every byte phase of the
caller's buffers.  Needs an MI355X: -m gpu.

Every batched kernel picks a vector or a byte path at run time from max_payload % 4 and from the
alignment of the caller's pointers (fec_codec.hip launch_encode / launch_copy, fec_kernels.hip,
fec_shapes.hip, fec_plan_fast.hip, fec_block.hip, fec_swdf.hip launch_fast / launch_tile,
fec_sdswdf.hip).  Here every buffer handed to the library is carved out of a larger allocation at a
chosen byte offset, with 256 guard bytes on both sides that must still hold their fill after the
call, and every result is compared with the oracle (tests/test_oracle.py pins the oracle at these
sizes on the CPU).  Each case asserts from the oracle alone, before the GPU is called, that its
inputs hold what it claims to exercise.

Branch each case reaches, from reading the code.  Global loads and stores may be unaligned on
gfx950; LDS and LDS-DMA accesses may not, and every LDS address below is 16-byte aligned by
construction (carve offsets rounded to 16, the misalignment carried as a byte offset `delta`).

  max_payload % 4 != 0    fec_encode_kernel with the byte scatter (no tile encoder), fec_copy_kernel
                          (no LDS-tile copy); recovery <17, staged>, <32, unstaged> at (10,9,1)
                          (n = 19), <17, unstaged> at L = 1499 (a span over 12 KB)
  encode, phase (0,0)     tile encoder under "auto"
  payload & 3 != 0        generic encoder, byte loads of the rows; "tile" refused
  codewords & 15 != 0     generic encoder, byte stores (uint4 only for a 16-byte aligned tile whose
                          byte count is a multiple of 16: P = 1 and R+1 end on other counts)
  decode, codewords & 15  the copy stages from the aligned address below and keeps the offset; the
                          staged recovery reads unaligned uint4 at a.cw + (s0 & ~15), inside the buffer
  flags & 15 != 0         episode scan: aligned 8-byte words (scalar loop for t < 8 and the last 72
                          packets); planners: dwords only where er + t is 4-byte aligned, else bytes
  out & 3 != 0            generic copy (byte stores); "fast" refused.  out & 15 != 0: dword stores
  block mode off phase    byte staging on the misaligned side
  relay type 2, L = 300   (10,3,10,3): the specialised kernels while the input is 16-byte and the
                          output 4-byte aligned (frames at 4, 8; destination rows at 4), else the
                          per-(packet, block) kernels; (10,3,9,2): the tile kernel while both are
                          16-byte aligned, else the per-(packet, block) kernels
  relay type 2, odd L     tile kernel ((10,3,10,3) at 299 / 301 has the blocks of 300 but not the
                          specialised kernels' payload size)
  relay type 3            tile kernel (16-byte buffer loads from the unaligned base, byte stores
                          where the output is not 16-byte aligned); per-(packet, block) kernel at L = 37
"""
import functools

import numpy as np
import pytest

import oracle
import test_oracle as cases  # the odd-size tuples, sizes and erasure pattern, pinned there on the CPU
from conftest import load_pattern

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402
from fec_erasure_code_unit_test_relay_amd._lib import FEC_ERR_ARG  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.relay import StateDependentRelay, SymbolWiseRelay  # noqa: E402

SEED = 0x5EED
GUARD = 256
IN_FILL, OUT_FILL = 0xA5, 0x5A
_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def carve(nbytes, off, dtype=torch.uint8, out=False):
    """A contiguous `nbytes` view that starts GUARD + off bytes into a fresh flat allocation (whose
    base is at least 256-byte aligned, so `off` is the view's byte phase), the whole allocation
    filled with 0xA5 (inputs) or 0x5A (outputs), and a checker that every byte outside the view
    still holds the fill."""
    fill = OUT_FILL if out else IN_FILL
    flat = torch.full((GUARD + off + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    lo, hi = GUARD + off, GUARD + off + nbytes
    view = flat[lo:hi]
    if dtype != torch.uint8:
        assert lo % 4 == 0 and nbytes % 4 == 0
        view = view.view(dtype)

    def check():
        assert bool((flat[:lo] == fill).all()), "bytes in front of the buffer were written"
        assert bool((flat[hi:] == fill).all()), "bytes behind the buffer were written"

    return view, check


def place(arr, off=0):
    """The host array `arr` (uint8 or int32) on the device at byte phase `off`, guards around it."""
    arr = np.ascontiguousarray(arr)
    view, _ = carve(arr.nbytes, off, _TORCH[arr.dtype])
    view = view.view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    return view


class Out:
    """An output buffer [shape] at byte phase `off` between guards."""

    def __init__(self, shape, off=0, dtype=torch.uint8):
        n = int(np.prod(shape)) * (4 if dtype == torch.int32 else 1)
        flat, self.check = carve(n, off, dtype, out=True)
        self.t = flat.view(shape)

    def host(self):
        self.check()
        return self.t.cpu().numpy()

    def untouched(self):
        self.check()
        fill = OUT_FILL if self.t.dtype == torch.uint8 else int.from_bytes(bytes([OUT_FILL] * 4), "little")
        return bool((self.t == fill).all())


def garbled(cw, pat, seed):
    """The codewords with the erased packets' rows replaced by random bytes (never read)."""
    cw = cw.copy()
    idx = np.flatnonzero(pat[:cw.shape[0]])
    cw[idx] = np.random.default_rng(seed).integers(0, 256, (idx.size, cw.shape[1]), dtype=np.uint8)
    return cw


def refused(fn):
    """fn() must be refused with FEC_ERR_ARG."""
    with pytest.raises(fec.FecError) as e:
        fn()
    assert e.value.status == FEC_ERR_ARG


def check_decode(c, out, ln, ref, pat, P, what):
    assert (ln.host() == ref["out_len"]).all(), what
    assert (out.host() == ref["out_data"]).all(), what
    eps, rec, lost = c.counters()
    assert lost == int((ref["out_len"] == 0).sum()), what  # every lost packet is an erased one
    assert rec + lost == int(pat[:P].sum()), what


# ---- payload sizes that are not whole dwords -----------------------------------------------------
ODD_CASES = [(tbn, L) for tbn in cases.ODD_TUPLES for L in cases.ODD_SIZES] + [((10, 3, 3), 1499)]
ODD_IDS = ["%d-%d-%d-L%d" % (*tbn, L) for tbn, L in ODD_CASES]
odd = pytest.mark.parametrize("tbn,L", ODD_CASES, ids=ODD_IDS)
P_ODD = cases.ODD_P


@functools.lru_cache(maxsize=None)
def odd_stream(tbn, L):
    """One oracle run per (tuple, size), shared by the tests below and left unchanged."""
    T, B, N = tbn
    pat = cases.odd_size_pattern(T, B)
    ref = oracle.run_stream(L, T, B, N, P_ODD, pat, seed=SEED, want_data=True, want_codewords=True)
    ok = ref["out_len"] > 0
    if B > 0:
        assert int((ok & (pat[:P_ODD] == 1)).sum()) >= 1, "no recovered packet"
    if tbn in cases.ODD_LOSSY:
        assert int((~ok).sum()) >= 1, "no lost packet"
    return pat, ref


def odd_lengths(L, rows, seed):
    lens = np.random.default_rng(seed).integers(0, L + 1, size=rows).astype(np.int32)
    lens[::7] = 0
    lens[1::11] = 1
    lens[2::5] = L
    assert {0, 1, L} <= set(lens.tolist())
    return lens


def oracle_encode(L, tbn, payload, lens):
    """A fresh FEC_Encoder of the oracle over the rows, one onTransmit per row."""
    enc = oracle.Encoder(L, *tbn)
    rows = [enc.onTransmit(payload[t], int(lens[t]), t) for t in range(payload.shape[0])]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.int32)


@odd
def test_odd_size_has_no_dword_kernels(tbn, L):
    """max_payload % 4 != 0: neither the tile encoder nor the LDS-tile copy exists; both planners do."""
    c = fec.Codec(L, *tbn)
    refused(lambda: c.set_encode_path("tile"))
    refused(lambda: c.set_copy_path("fast"))
    c.set_plan_path("generic")
    c.set_plan_path("auto")
    info = c.info()
    assert info["encode_kernel"] == "fec_encode_kernel" and info["copy_kernel"] == "fec_copy_kernel"
    assert (info["k"], info["n"], info["S"], info["CW"]) == oracle.geometry(L, *tbn)


@odd
def test_odd_size_encode_vs_oracle_stream(tbn, L):
    T = tbn[0]
    rows = P_ODD + T
    ref = oracle.encode_stream(L, *tbn, 0, rows, seed=SEED)
    c = fec.Codec(L, *tbn)
    for path in ("auto", "generic"):
        c.set_encode_path(path)
        cw, wl = Out((rows, c.CW)), Out((rows,), dtype=torch.int32)
        c.encode(place(oracle.fill_payload(0, rows, L, SEED)), out=cw.t, out_len=wl.t)
        assert (cw.host() == ref["cw"]).all(), path
        assert (wl.host() == ref["cw_len"]).all(), path


@odd
def test_odd_size_encode_lengths_and_history(tbn, L):
    """Random lengths that hold 0, 1 and L; the stream in two batches, the second with 0, 1 and n-1
    rows of history: the rows before the history count as zero, so the expected codewords are a
    fresh oracle encoder's over the history and the batch."""
    rows, cut = P_ODD + tbn[0], 200
    lens = odd_lengths(L, rows, L + sum(tbn))
    payload = oracle.fill_payload(0, rows, L, 9)
    c = fec.Codec(L, *tbn)
    ref, ref_wl = oracle_encode(L, tbn, payload, lens)
    cw, wl = Out((rows, c.CW)), Out((rows,), dtype=torch.int32)
    c.encode(place(payload), place(lens), out=cw.t, out_len=wl.t)
    assert (cw.host() == ref).all() and (wl.host() == ref_wl).all()
    for h in (0, 1, c.n - 1):
        want, want_wl = oracle_encode(L, tbn, payload[cut - h:], lens[cut - h:])
        cw, wl = Out((rows - cut, c.CW)), Out((rows - cut,), dtype=torch.int32)
        c.encode(place(payload[cut - h:]), place(lens[cut - h:]), history=h, out=cw.t, out_len=wl.t)
        assert (cw.host() == want[h:]).all() and (wl.host() == want_wl[h:]).all(), h
        if h == c.n - 1:  # a parity symbol reaches n-1 packets back at most: the one-batch rows
            assert (want[h:] == ref[cut:]).all()


@odd
def test_odd_size_decode_vs_oracle(tbn, L):
    T = tbn[0]
    pat, ref = odd_stream(tbn, L)
    c = fec.Codec(L, *tbn)
    cw = place(garbled(ref["cw"], pat, L))
    er = place(pat)
    for plan in ("generic", "auto"):
        for dedup in (True, False):
            c.set_plan_path(plan)
            c.set_episode_dedup(dedup)
            out, ln = Out((P_ODD, L)), Out((P_ODD,), dtype=torch.int32)
            c.decode(cw, er, out=out.t, out_len=ln.t)
            check_decode(c, out, ln, ref, pat, P_ODD, (plan, dedup))


@pytest.mark.parametrize("tbn", [(10, 3, 3), (10, 10, 10)])
@pytest.mark.parametrize("L", [37, 301])
def test_odd_size_decode_variable_lengths(tbn, L):
    """Packets of every length through the decode, against the oracle's FEC_Decoder fed the same
    stream packet by packet."""
    T, B, N = tbn
    rows = P_ODD + T
    pat = cases.odd_size_pattern(T, B)
    lens = odd_lengths(L, rows, L)
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
    erased = pat[:P_ODD] == 1
    assert (want_len[erased & (lens[:P_ODD] > 0)] > 0).any(), "no recovered packet"
    c = fec.Codec(L, T, B, N)
    cw, er = place(garbled(np.stack(cws), pat, L)), place(pat)
    for cpath in ("auto", "generic"):
        c.set_copy_path(cpath)
        out, ln = Out((P_ODD, L)), Out((P_ODD,), dtype=torch.int32)
        c.decode(cw, er, out=out.t, out_len=ln.t)
        assert (ln.host() == want_len).all(), cpath
        assert (out.host() == want).all(), cpath


def test_odd_size_continuing_decode():
    """DecodeStream.push at L = 37: pushes of 1, 2, 11, 64 and 250 packets, the whole stream kept as
    history, against the one oracle run."""
    tbn, L = (10, 3, 3), 37
    T = tbn[0]
    pat, ref = odd_stream(tbn, L)
    c = fec.Codec(L, *tbn)
    cw, er = place(garbled(ref["cw"], pat, L)), place(pat)
    ds = fec.DecodeStream(c)
    outs, lens, a = [], [], 0
    sizes = [1, 2, 11, 64, 250]
    for i in range(1000):
        if a >= P_ODD + T:
            break
        b = min(P_ODD + T, a + sizes[i % len(sizes)])
        out, ln = Out((b - a, L)), Out((b - a,), dtype=torch.int32)
        o, n = ds.push(cw[:b], er[:b], pat[:b], history=a, out=out.t, out_len=ln.t)
        torch.cuda.synchronize()
        out.check()
        ln.check()
        outs.append(o.cpu().numpy())
        lens.append(n.cpu().numpy())
        a = b
    assert ds.state()[0] == P_ODD + T
    assert (np.concatenate(lens) == ref["out_len"]).all()
    assert (np.concatenate(outs) == ref["out_data"]).all()


# ---- every buffer phase, L = 300 and L = 64 -----------------------------------------------------
PHASE_SIZES = [300, 64]
ENC_PHASES = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 4), (0, 8), (0, 15), (3, 7)]  # (payload, codewords)
ENC_ROWS = 2500


@functools.lru_cache(maxsize=None)
def encode_refs(tbn, L):
    """One stream of n-1 + 2500 rows, with and without a length array, as device tensors."""
    k, n, S, CW = oracle.geometry(L, *tbn)
    rows = n - 1 + ENC_ROWS
    payload = oracle.fill_payload(0, rows, L, SEED)
    lens = odd_lengths(L, rows, 3)
    full = oracle.encode_stream(L, *tbn, 0, rows, seed=SEED)
    var = oracle_encode(L, tbn, payload, lens)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return payload, lens, {False: (dev(full["cw"]), dev(full["cw_len"])), True: (dev(var[0]), dev(var[1]))}


@pytest.mark.parametrize("L", PHASE_SIZES)
@pytest.mark.parametrize("tbn", [(10, 3, 3), (10, 10, 10), (10, 0, 0)])
def test_encode_at_every_buffer_phase(tbn, L):
    """Payload and codeword buffers at each byte phase, with and without a length array, with 0
    and n-1 rows of history inside the same buffer, automatic and generic kernel, batch sizes whose
    last tile ends on different byte counts.  With h rows of history the batch is rows h.. of the
    stream that starts at the buffer's first row, so the expected rows are that stream's."""
    payload, lens, refs = encode_refs(tbn, L)
    c = fec.Codec(L, *tbn)
    try:
        c.set_encode_path("tile")
        have_tile = True
    except fec.FecError as e:
        assert e.status == FEC_ERR_ARG
        have_tile = False
    R = c.info()["encode_tile_packets"]
    assert have_tile == (R > 0)
    for poff, coff in ENC_PHASES:
        for P in sorted({1, R + 1, ENC_ROWS}):
            for h in (0, c.n - 1):
                pay = place(payload[:h + P], poff)
                for with_len in (False, True):
                    dl = place(lens[:h + P]) if with_len else None
                    want, want_wl = refs[with_len]
                    for path in ("auto", "generic"):
                        c.set_encode_path(path)
                        cw, wl = Out((P, c.CW), coff), Out((P,), dtype=torch.int32)
                        c.encode(pay, dl, history=h, out=cw.t, out_len=wl.t)
                        what = (poff, coff, P, h, with_len, path)
                        cw.check()
                        wl.check()
                        assert torch.equal(cw.t, want[h:h + P]), what
                        assert torch.equal(wl.t, want_wl[h:h + P]), what
        if have_tile and (poff & 3 or coff & 15):
            # a phase the tile kernel excludes: refused before any launch
            c.set_encode_path("tile")
            cw, wl = Out((R + 1, c.CW), coff), Out((R + 1,), dtype=torch.int32)
            refused(lambda: c.encode(place(payload[:R + 1], poff), out=cw.t, out_len=wl.t))
            torch.cuda.synchronize()
            assert cw.untouched() and wl.untouched(), (poff, coff)


DEC_ROWS = 1500
# (codewords, erasure flags, payload output) phases: every value of an axis with the other two at 0,
# and three mixed points
DEC_PHASES = ([(0, 0, 0)] + [(c, 0, 0) for c in (1, 2, 5, 8, 15)] + [(0, e, 0) for e in (1, 7, 9, 15)] +
              [(0, 0, o) for o in (1, 2, 3, 4, 8)] + [(5, 9, 3), (15, 15, 1), (1, 7, 2)])


def phase_pattern(T, B, P=DEC_ROWS):
    """P + T flags: 3 % i.i.d. loss, erasures at t < 8 and inside the last 72 packets (the scalar
    branches of the episode scan's flag words), a burst of B+1."""
    rng = np.random.default_rng(0xFA5E)
    pat = (rng.random(P + T) < 0.03).astype(np.uint8)
    pat[[2, 5]] = 1
    pat[700:700 + B + 1] = 1
    pat[1100:1103] = 1
    pat[[P + T - 40, P + T - 12, P + T - 11]] = 1
    return pat


@functools.lru_cache(maxsize=None)
def phase_stream(tbn, L):
    T, B, N = tbn
    pat = phase_pattern(T, B)
    ref = oracle.run_stream(L, T, B, N, DEC_ROWS, pat, seed=SEED, want_data=True, want_codewords=True)
    ok = ref["out_len"] > 0
    assert pat[:8].any() and pat[DEC_ROWS + T - 72:].any()
    assert int((ok & (pat[:DEC_ROWS] == 1)).sum()) >= 1, "no recovered packet"
    if tbn == (10, 3, 3):
        assert int((~ok).sum()) >= 1, "no lost packet"
    return pat, ref, garbled(ref["cw"], pat, L)


@pytest.mark.parametrize("L", PHASE_SIZES)
@pytest.mark.parametrize("tbn", [(10, 3, 3), (10, 10, 10)])
def test_decode_at_every_buffer_phase(tbn, L):
    pat, ref, noisy = phase_stream(tbn, L)
    P = DEC_ROWS
    c = fec.Codec(L, *tbn)
    assert c.info()["copy_kernel"].startswith(("fec_copy_pair_kernel", "fec_copy_fast_kernel"))
    for coff, eoff, ooff in DEC_PHASES:
        cw, er = place(noisy, coff), place(pat, eoff)
        both = ("auto", "generic") if (coff, eoff, ooff) in ((0, 0, 0), (15, 0, 0)) else ("auto",)
        for cpath in both:
            for ppath in both:
                c.set_copy_path(cpath)
                c.set_plan_path(ppath)
                out, ln = Out((P, L), ooff), Out((P,), dtype=torch.int32)
                c.decode(cw, er, out=out.t, out_len=ln.t)
                check_decode(c, out, ln, ref, pat, P, (coff, eoff, ooff, cpath, ppath))
        if ooff & 3:  # the LDS-tile copy stores dwords: refused before it writes anything
            c.set_copy_path("fast")
            out, ln = Out((P, L), ooff), Out((P,), dtype=torch.int32)
            refused(lambda: c.decode(cw, er, out=out.t, out_len=ln.t))
            torch.cuda.synchronize()
            assert out.untouched() and ln.untouched(), (coff, eoff, ooff)
            c.set_copy_path("auto")


@pytest.mark.parametrize("L", PHASE_SIZES)
@pytest.mark.parametrize("tbn", [(10, 3, 3), (10, 10, 10)])
def test_split_decode_at_a_misaligned_phase(tbn, L):
    """plan + apply and plan + copy + recover at phase (5, 9, 3) equal the one-shot decode, which is
    itself compared with the oracle here."""
    pat, ref, noisy = phase_stream(tbn, L)
    P = DEC_ROWS
    c = fec.Codec(L, *tbn)
    cw, er = place(noisy, 5), place(pat, 9)
    out, ln = Out((P, L), 3), Out((P,), dtype=torch.int32)
    c.decode(cw, er, out=out.t, out_len=ln.t)
    check_decode(c, out, ln, ref, pat, P, "one shot")
    out2, ln2 = Out((P, L), 3), Out((P,), dtype=torch.int32)
    c.plan(er)
    c.apply(cw, er, out=out2.t, out_len=ln2.t)
    check_decode(c, out2, ln2, ref, pat, P, "plan + apply")
    assert torch.equal(out2.t, out.t) and torch.equal(ln2.t, ln.t)
    out3, ln3 = Out((P, L), 3), Out((P,), dtype=torch.int32)
    c.plan(er)
    c.copy(cw, er, out=out3.t, out_len=ln3.t)
    c.recover(cw, out3.t, ln3.t)
    check_decode(c, out3, ln3, ref, pat, P, "plan + copy + recover")
    assert torch.equal(out3.t, out.t) and torch.equal(ln3.t, ln.t)


@pytest.mark.parametrize("tbn", [(10, 3, 3), (6, 4, 2)])
def test_block_mode_at_misaligned_phases(tbn):
    """encode_blocks with data and out, decode_blocks with codewords and flags, off the dword
    phase: block counts around the 256-block stage, every erasure mask of the code."""
    c = fec.Codec(300, *tbn)
    k, n = c.k, c.n
    assert n <= 11
    G = oracle.gen_G(*tbn)
    rng = np.random.default_rng(7)

    def enc_ref(data):
        ref = np.zeros((data.shape[0], n), dtype=np.uint8)
        ref[:, :k] = data  # the relay pre-fills the codeword with the data
        for b in range(data.shape[0]):
            oracle.encode_block(data[b], G, ref[b], k - 1)
        return ref

    for nblk in (1, 255, 256):
        data = rng.integers(0, 256, (nblk, k), dtype=np.uint8)
        ref = enc_ref(data)
        assert (ref[:, k:] != 0).any()
        for off in (1, 2, 3):
            out = Out((nblk, n), off)
            c.encode_blocks(place(data, off), out=out.t)
            assert (out.host() == ref).all(), (nblk, off)
    masks = np.arange(1 << n, dtype=np.int64)
    er = ((masks[:, None] >> np.arange(n)) & 1).astype(np.uint8)
    data = rng.integers(0, 256, (masks.size, k), dtype=np.uint8)
    noisy = enc_ref(data)
    noisy[er == 1] = rng.integers(0, 256, int(er.sum()), dtype=np.uint8)  # erased symbols: garbage
    want = [oracle.decode_block(noisy[b], G, er[b], n - 1, 0) for b in range(masks.size)]
    want_cw, want_er = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert ((er[:, :k] == 1) & (want_er[:, :k] == 0)).any(), "no recovered symbol"
    for off in (1, 3):
        out, er_out = c.decode_blocks(place(noisy, off), place(er, off))
        assert (out.cpu().numpy() == want_cw).all() and (er_out.cpu().numpy() == want_er).all(), off


# ---- fixed-rate relay ------------------------------------------------------------------------------
RELAY_ROWS = 600


@functools.lru_cache(maxsize=None)
def relay_hops():
    """The hop patterns and forced erasures of test_swdf.test_gpu_swdf_bit_exact_vs_oracle at 600 packets."""
    P = RELAY_ROWS
    e1 = load_pattern("bin_erasure")[3000:3000 + P].copy()
    e2 = load_pattern("bin_erasure2")[9000:9000 + P].copy()
    e1[[0, 1, 2, 3, 500, 501, 503, 505, 507]] = 1  # start-up and dense windows
    e2[[5, 6, 400, 402, 404, 406]] = 1
    return e1, e2


@functools.lru_cache(maxsize=None)
def relay_case(cfg, L, kind):
    """(source codewords with erased rows garbled, oracle run with its frames garbled for hop 2)."""
    P = RELAY_ROWS
    e1, e2 = relay_hops()
    run = oracle.swdf_run if kind == 2 else oracle.sdswdf_run
    ref = run(L, *cfg, P, e1, e2, seed=SEED)
    T1, N1 = cfg[:2]
    src = oracle.encode_stream(L, T1, N1, N1, 0, P, seed=SEED)["cw"]
    if kind == 2:
        assert ref["relay_flag"].sum() > 0
        assert ref["dest_flag"].sum() > 0 or cfg[3] >= 6  # (6,2,10,6): hop 2 corrects every window
        if cfg == (10, 3, 10, 3):  # both failure paths: the counts of the shipped patterns' windows
            assert ref["relay_flag"].sum() == 60 and ref["dest_flag"].sum() == 41
    else:
        assert ref["dest_flag"].sum() > 0
    return garbled(src, e1, L), garbled(ref["frames"], e2, L + 1), ref


def run_type2(cfg, L, cw_off=0, fr_off=0, out_off=0):
    """Relay and destination legs, each fed from the oracle (source codewords; the oracle's frames)
    and compared with it.  fr_off is the phase of the relay's frame output and of the destination's
    frame input."""
    P = RELAY_ROWS
    e1, e2 = relay_hops()
    src, fr_in, ref = relay_case(cfg, L, 2)
    r = SymbolWiseRelay(L, *cfg)
    assert r.delay == ref["delay"] and r.frame_bytes == ref["frames"].shape[1]
    what = (cfg, L, cw_off, fr_off, out_off)
    frames, rflag = Out((P, r.frame_bytes), fr_off), Out((P,))
    r.relay(place(src, cw_off), place(e1), frames=frames.t, flag=rflag.t)
    assert (frames.host() == ref["frames"]).all(), what
    assert (rflag.host() == ref["relay_flag"]).all(), what
    out, dflag = Out((P, r.S * r.k), out_off), Out((P,))
    r.destination(place(fr_in, fr_off), place(e2), out=out.t, flag=dflag.t)
    assert (out.host() == ref["dest_out"]).all(), what
    assert (dflag.host() == ref["dest_flag"]).all(), what


@pytest.mark.parametrize("L", [37, 299, 301])
@pytest.mark.parametrize("cfg", [(10, 3, 10, 3), (10, 3, 9, 2), (6, 2, 10, 6)])
def test_relay_type2_at_odd_payload_sizes(cfg, L):
    """299 and 301 give the S = 38 blocks of 300 at (10,3,10,3) but are not the specialised
    kernels' payload size: the runtime-K tile kernel."""
    run_type2(cfg, L)


# one axis at a time, and one mixed point: (codewords, frames, destination output)
RELAY_PHASES = ([(0, 0, 0)] + [(c, 0, 0) for c in (1, 4, 8)] + [(0, f, 0) for f in (1, 4, 8)] +
                [(0, 0, o) for o in (1, 2, 4)] + [(1, 4, 2)])


@pytest.mark.parametrize("cfg", [(10, 3, 10, 3), (10, 3, 9, 2)])
def test_relay_type2_at_misaligned_phases(cfg):
    """L = 300.  (10,3,10,3) is the specialised tier (16-byte aligned input, 4-byte aligned output),
    (10,3,9,2) the tile tier (both 16-byte aligned); any other phase falls through to the
    per-(packet, block) kernels (fec_swdf.hip launch_fast / launch_tile)."""
    for cw_off, fr_off, out_off in RELAY_PHASES:
        run_type2(cfg, 300, cw_off, fr_off, out_off)


@pytest.mark.parametrize("L,off", [(37, 0), (301, 0), (300, 1), (300, 4)])
def test_relay_type3_odd_sizes_and_misaligned_phases(L, off):
    cfg = (10, 3, 10, 3)
    P = RELAY_ROWS
    e1, e2 = relay_hops()
    src, fr_in, ref = relay_case(cfg, L, 3)
    r = StateDependentRelay(L, *cfg)
    assert r.delay == ref["delay"] and r.frame_bytes == ref["frames"].shape[1]
    frames = Out((P, r.frame_bytes), off)
    r.relay(place(src, off), e1, frames=frames.t)
    assert (frames.host() == ref["frames"]).all()
    out = Out((P, r.S * r.k), off)
    _, dflag = r.destination(place(fr_in, off), e2, out=out.t)
    assert (out.host() == ref["dest_out"]).all()
    assert (dflag == ref["dest_flag"]).all()
