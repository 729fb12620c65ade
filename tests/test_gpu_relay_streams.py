"""Relay stream groups (fec_relay_streams_*) on the GPU: per stream, the rows of all relay and
destination calls together -- one-packet calls and bursts of any size in any cutting -- equal the
oracle's SWDF chain (or_swdf_run) and the batched SymbolWiseRelay over that stream's whole sequence
from seq 0, byte for byte.  Needs an MI355X: -m gpu."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from conftest import load_pattern
from test_swdf import SWDF_CASES

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.relay import RelayStreamGroup, SymbolWiseRelay  # noqa: E402

SEED = 0x5EED
NS = 5
E1_SET = [0, 1, 2, 3, 60, 61, 63, 65, 67, 90]
E2_SET = [5, 6, 80, 82, 84, 86, 110]

CASES = [(cfg, 300, 300) for cfg in SWDF_CASES] + [((10, 3, 10, 3), 1000, 120)]
CASE_IDS = ["cfg%d" % i for i in range(len(SWDF_CASES))] + ["cfg0-L1000"]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def hop_patterns(m, P):
    e1 = load_pattern("bin_erasure")[3000 + 997 * m:3000 + 997 * m + P].astype(np.uint8)
    e2 = load_pattern("bin_erasure2")[9000 + 1013 * m:9000 + 1013 * m + P].astype(np.uint8)
    e1[E1_SET] = 1
    e2[E2_SET] = 1
    return e1, e2


def garbled(rows, erasure):
    """A copy of `rows` with the rows of erased packets overwritten: they must never be read."""
    g = rows.clone()
    idx = torch.nonzero(torch.from_numpy(erasure.astype(bool)).to(rows.device)).flatten()
    g[idx] = torch.randint(0, 256, (idx.numel(), rows.shape[1]), dtype=torch.uint8, device=rows.device)
    return g


class Chains:
    """NS independent chains of one case: hop patterns, the source's codewords (erased rows garbled)
    and the oracle's run per stream.  Built once per case and left unchanged."""

    def __init__(self, cfg, L, P):
        T1, N1, T2, N2 = cfg
        self.cfg, self.L, self.P = cfg, L, P
        self.k, self.n1, self.n2 = T1 - N1 + 1, T1 + 1, T2 + 1
        c = fec.Codec(L, T1, N1, N1)
        self.e1, self.e2, self.cw, self.ref = [], [], [], []
        for m in range(NS):
            e1, e2 = hop_patterns(m, P)
            cw, _ = c.encode(fec.fill_payload(0, P, L, SEED + m))
            self.e1.append(e1)
            self.e2.append(e2)
            self.cw.append(garbled(cw, e1))
            self.ref.append(oracle.swdf_run(L, *cfg, P, e1, e2, seed=SEED + m))
        torch.cuda.synchronize()

    def recovered_windows(self, e, n):
        pad = np.concatenate([np.zeros(n - 1, dtype=np.int64), e.astype(np.int64)])
        cnt = np.convolve(pad, np.ones(n, dtype=np.int64), mode="valid")
        return int(((cnt > 0) & (cnt < n - self.k + 1)).sum())

    def assert_exercised(self):
        """The reference itself covers recovery on both hops in every stream, the relay's failure
        flag in every case and the destination's wherever the code does not absorb the pattern."""
        for m in range(NS):
            assert self.recovered_windows(self.e1[m], self.n1) >= 16, m
            assert self.recovered_windows(self.e2[m], self.n2) >= 16, m
        rflags = [int(r["relay_flag"].sum()) for r in self.ref]
        dflags = [int(r["dest_flag"].sum()) for r in self.ref]
        assert sum(rflags) > 0
        if self.cfg == (10, 10, 10, 10):
            assert rflags == [0, 0, 0, 1, 0]
        if self.cfg in ((10, 10, 10, 10), (6, 2, 10, 6)):
            assert sum(dflags) == 0
        else:
            assert sum(dflags) > 0


@functools.lru_cache(maxsize=None)
def chains(cfg, L, P):
    return Chains(cfg, L, P)


def cut(ns, P, rng, choices):
    """A random cutting of ns streams of P seqs into calls: (ids, counts or None, [(stream, first
    seq, count)]) -- a random permuted subset of the live streams per call, half the calls
    one-packet calls (counts None)."""
    sent = np.zeros(ns, dtype=np.int64)
    while (sent < P).any():
        live = np.flatnonzero(sent < P)
        ids = rng.permutation(live)[:max(1, int(rng.integers(1, live.size + 1)))].astype(np.int32)
        single = rng.random() < 0.5
        counts = np.array([1 if single else min(int(rng.choice(choices)), P - sent[s]) for s in ids], dtype=np.int32)
        yield ids, (None if single else counts), [(int(s), int(sent[s]), int(c)) for s, c in zip(ids, counts)]
        sent[ids] += counts


def run_side(call, rows_in, flags_in, width, ns, P, rng, choices):
    """Feed every stream's P rows through `call` in a random cutting; the outputs per stream."""
    dev = rows_in[0].device
    out = torch.zeros((ns, P, width), dtype=torch.uint8, device=dev)
    flag = torch.zeros((ns, P), dtype=torch.uint8, device=dev)
    for ids, counts, parts in cut(ns, P, rng, choices):
        x = torch.cat([rows_in[s][a:a + c] for s, a, c in parts])
        er = np.concatenate([flags_in[s][a:a + c] for s, a, c in parts])
        o, f = call(ids, counts, er, x)
        row = 0
        for s, a, c in parts:
            out[s, a:a + c], flag[s, a:a + c] = o[row:row + c], f[row:row + c]
            row += c
    return out, flag


def burst_choices(n1, n2):
    return sorted({1, 2, n1 - 1, n1, n1 + 1, n1 + n2 - 2, n1 + n2 - 1, 31, 32, 33, 70})


def drive_both(grp, e1, e2, cws, rng, ns, P):
    """Relay pass, then (another cutting) the destination pass over the frames with the rows of
    hop-2 erasures garbled; returns frames, relay flags, destination rows, destination flags."""
    choices = burst_choices(grp.n1, grp.n2)
    frames, rflag = run_side(grp.relay, cws, e1, grp.frame_bytes, ns, P, rng, choices)
    rx = [garbled(frames[s], e2[s]) for s in range(ns)]
    out, dflag = run_side(grp.destination, rx, e2, grp.S * grp.k, ns, P, rng, choices)
    torch.cuda.synchronize()
    for s in range(ns):
        assert grp.state(s) == (P, P), s
    return frames, rflag, out, dflag


def assert_equals_oracle(got, ref, s, rows=slice(None)):
    frames, rflag, out, dflag = got
    assert (rflag.cpu().numpy() == ref["relay_flag"][rows]).all(), s
    assert (frames.cpu().numpy() == ref["frames"][rows]).all(), s
    assert (dflag.cpu().numpy() == ref["dest_flag"][rows]).all(), s
    assert (out.cpu().numpy() == ref["dest_out"][rows]).all(), s


@pytest.mark.parametrize("cfg,L,P", CASES, ids=CASE_IDS)
def test_group_equals_oracle_per_stream(cfg, L, P):
    ch = chains(cfg, L, P)
    ch.assert_exercised()
    grp = RelayStreamGroup(L, *cfg, NS)
    assert (grp.k, grp.n1, grp.n2) == (ch.k, ch.n1, ch.n2)
    assert grp.delay == ch.ref[0]["delay"] and grp.frame_bytes == ch.ref[0]["frames"].shape[1]
    assert grp.cw_bytes == ch.cw[0].shape[1]
    rng = np.random.default_rng(53)
    frames, rflag, out, dflag = drive_both(grp, ch.e1, ch.e2, ch.cw, rng, NS, P)
    for s in range(NS):
        assert_equals_oracle((frames[s], rflag[s], out[s], dflag[s]), ch.ref[s], s)


def test_group_equals_batch_for_short_payloads():
    """Payload sizes 0..L (0 and L among them): every stream equals the batched relay and
    destination over that stream alone."""
    cfg, L, P = (10, 3, 10, 3), 300, 300
    rng = np.random.default_rng(59)
    c = fec.Codec(L, 10, 3, 3)
    batch = SymbolWiseRelay(L, *cfg)
    e1, e2, cws, want = [], [], [], []
    for m in range(NS):
        a, b = hop_patterns(m, P)
        ln = rng.integers(0, L + 1, P).astype(np.int32)
        ln[rng.integers(0, P, 8)] = 0
        ln[rng.integers(0, P, 8)] = L
        cw, _ = c.encode(fec.fill_payload(0, P, L, SEED + m), torch.from_numpy(ln).cuda())
        cw = garbled(cw, a)
        fr, rf = batch.relay(cw, torch.from_numpy(a).cuda())
        rx = garbled(fr, b)
        o, df = batch.destination(rx, torch.from_numpy(b).cuda())
        e1.append(a), e2.append(b), cws.append(cw), want.append((fr, rf, o, df, rx))
    grp = RelayStreamGroup(L, *cfg, NS)
    choices = burst_choices(grp.n1, grp.n2)
    frames, rflag = run_side(grp.relay, cws, e1, grp.frame_bytes, NS, P, rng, choices)
    out, dflag = run_side(grp.destination, [w[4] for w in want], e2, grp.S * grp.k, NS, P, rng, choices)
    torch.cuda.synchronize()
    for s in range(NS):
        fr, rf, o, df, _ = want[s]
        assert torch.equal(rflag[s], rf) and torch.equal(frames[s], fr), s
        assert torch.equal(dflag[s], df) and torch.equal(out[s], o), s


def test_one_long_burst():
    """One stream, 2 000 seqs in one call (many chunks, one workgroup each), then 40 one-packet
    calls: equal to the batched path over all 2 040 seqs."""
    cfg, L, Q, tail = (10, 3, 10, 3), 300, 2000, 40
    P = Q + tail
    e1, e2 = hop_patterns(1, P)
    c = fec.Codec(L, 10, 3, 3)
    cw, _ = c.encode(fec.fill_payload(0, P, L, SEED))
    cw = garbled(cw, e1)
    batch = SymbolWiseRelay(L, *cfg)
    fr, rf = batch.relay(cw, torch.from_numpy(e1).cuda())
    rx = garbled(fr, e2)
    o, df = batch.destination(rx, torch.from_numpy(e2).cuda())
    grp = RelayStreamGroup(L, *cfg, 1)
    ids = np.zeros(1, dtype=np.int32)
    got_fr, got_rf = [], []
    a, b = grp.relay(ids, np.array([Q], dtype=np.int32), e1[:Q], cw[:Q])
    got_fr.append(a), got_rf.append(b)
    for t in range(Q, P):
        a, b = grp.relay(ids, None, e1[t:t + 1], cw[t:t + 1])
        got_fr.append(a), got_rf.append(b)
    got_o, got_df = [], []
    a, b = grp.destination(ids, np.array([Q], dtype=np.int32), e2[:Q], rx[:Q])
    got_o.append(a), got_df.append(b)
    for t in range(Q, P):
        a, b = grp.destination(ids, None, e2[t:t + 1], rx[t:t + 1])
        got_o.append(a), got_df.append(b)
    torch.cuda.synchronize()
    assert grp.state(0) == (P, P)
    assert torch.equal(torch.cat(got_rf), rf) and torch.equal(torch.cat(got_fr), fr)
    assert torch.equal(torch.cat(got_df), df) and torch.equal(torch.cat(got_o), o)


def test_calls_on_two_streams_are_ordered():
    """Calls alternate between two HIP streams with no synchronisation between them: the group
    orders its staging and rings itself, so every row still equals the oracle's."""
    cfg, L, P = SWDF_CASES[0], 300, 300
    ch = chains(cfg, L, P)
    grp = RelayStreamGroup(L, *cfg, NS)
    Q = 12
    rounds = P // Q
    ids = np.arange(NS, dtype=np.int32)
    counts = np.full(NS, Q, dtype=np.int32)
    cw_r = [torch.cat([ch.cw[s][r * Q:(r + 1) * Q] for s in range(NS)]) for r in range(rounds)]
    e1_r = [np.concatenate([ch.e1[s][r * Q:(r + 1) * Q] for s in range(NS)]) for r in range(rounds)]
    e2_r = [np.concatenate([ch.e2[s][r * Q:(r + 1) * Q] for s in range(NS)]) for r in range(rounds)]
    frames = torch.zeros((rounds, NS * Q, grp.frame_bytes), dtype=torch.uint8, device="cuda")
    rflag = torch.zeros((rounds, NS * Q), dtype=torch.uint8, device="cuda")
    out = torch.zeros((rounds, NS * Q, grp.S * grp.k), dtype=torch.uint8, device="cuda")
    dflag = torch.zeros((rounds, NS * Q), dtype=torch.uint8, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r in range(rounds):
        with torch.cuda.stream(streams[r % 2]):
            grp.relay(ids, counts, e1_r[r], cw_r[r], frames=frames[r], flag=rflag[r])
    torch.cuda.synchronize()
    rx = [garbled(frames[r], e2_r[r]) for r in range(rounds)]
    torch.cuda.synchronize()
    for r in range(rounds):
        with torch.cuda.stream(streams[(r + 1) % 2]):
            grp.destination(ids, counts, e2_r[r], rx[r], out=out[r], flag=dflag[r])
    torch.cuda.synchronize()

    def per_stream(x, s):
        return x.view(rounds, NS, Q, -1)[:, s].reshape(rounds * Q, -1)

    for s in range(NS):
        got = (per_stream(frames, s), per_stream(rflag, s)[:, 0], per_stream(out, s), per_stream(dflag, s)[:, 0])
        assert_equals_oracle(got, ch.ref[s], s, slice(0, rounds * Q))


def test_bad_arguments_leave_group_unchanged():
    cfg, L, P = SWDF_CASES[0], 300, 300
    ch = chains(cfg, L, P)
    ns, first = 4, 50
    grp = RelayStreamGroup(L, *cfg, ns)
    ARG = fec._lib.FEC_ERR_ARG
    ids = np.array([2, 0, 1], dtype=np.int32)
    counts = np.full(3, first, dtype=np.int32)
    fr0, _ = grp.relay(ids, counts, np.concatenate([ch.e1[s][:first] for s in ids]),
                       torch.cat([ch.cw[s][:first] for s in ids]))
    grp.destination(ids, counts, np.concatenate([ch.e2[s][:first] for s in ids]),
                    torch.cat([garbled(fr0[j * first:(j + 1) * first], ch.e2[s][:first]) for j, s in enumerate(ids)]))
    torch.cuda.synchronize()
    before = [grp.state(s) for s in range(ns)]
    assert before == [(first, first)] * 3 + [(0, 0)]
    bad = [(np.array([3, 3], dtype=np.int32), np.array([2, 2], dtype=np.int32)),   # a repeated id
           (np.array([1, ns], dtype=np.int32), np.array([2, 2], dtype=np.int32)),  # an id out of range
           (np.array([1, -1], dtype=np.int32), None),
           (np.array([1, 2], dtype=np.int32), np.array([4, 0], dtype=np.int32))]   # a count of 0
    for b_ids, b_counts in bad:
        R = b_ids.size if b_counts is None else int(b_counts.sum())
        cw = torch.zeros((R, grp.cw_bytes), dtype=torch.uint8, device="cuda")
        fr = torch.zeros((R, grp.frame_bytes), dtype=torch.uint8, device="cuda")
        with pytest.raises(fec.FecError) as e:
            grp.relay(b_ids, b_counts, np.zeros(R, dtype=np.uint8), cw)
        assert e.value.status == ARG
        with pytest.raises(fec.FecError) as e:
            grp.destination(b_ids, b_counts, np.zeros(R, dtype=np.uint8), fr)
        assert e.value.status == ARG
        assert [grp.state(s) for s in range(ns)] == before
    # a row stride below S*n1, and null pointers: refused by the library before any launch
    one = np.array([1], dtype=np.int32)
    er = np.zeros(1, dtype=np.uint8)
    cw = torch.zeros((1, grp.cw_bytes), dtype=torch.uint8, device="cuda")
    fr = torch.zeros((1, grp.frame_bytes), dtype=torch.uint8, device="cuda")
    vp = ctypes.c_void_p
    relay = fec.lib().fec_relay_streams_relay
    assert relay(grp._h, one.ctypes.data_as(vp), None, 1, er.ctypes.data_as(vp), vp(cw.data_ptr()), grp.cw_bytes - 1,
                 vp(fr.data_ptr()), None, None) == ARG
    assert relay(grp._h, one.ctypes.data_as(vp), None, 1, er.ctypes.data_as(vp), None, grp.cw_bytes,
                 vp(fr.data_ptr()), None, None) == ARG
    assert relay(grp._h, one.ctypes.data_as(vp), None, 1, None, vp(cw.data_ptr()), grp.cw_bytes,
                 vp(fr.data_ptr()), None, None) == ARG
    assert [grp.state(s) for s in range(ns)] == before
    # a geometry whose smallest chunk does not fit a CU's LDS
    with pytest.raises(fec.FecError) as e:
        RelayStreamGroup(1500, 16, 16, 16, 16, 2)
    assert e.value.status == ARG
    # the next valid call continues every stream; its codeword rows start at an odd address
    more = 70
    R = 3 * more
    buf = torch.zeros(R * grp.cw_bytes + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(R, grp.cw_bytes)
    assert odd.data_ptr() % 2 == 1
    odd.copy_(torch.cat([ch.cw[s][first:first + more] for s in ids]))
    counts = np.full(3, more, dtype=np.int32)
    e1 = np.concatenate([ch.e1[s][first:first + more] for s in ids])
    try:
        frames, rflag = grp.relay(ids, counts, e1, odd)
    except fec.FecError as err:  # an alignment requirement, stated and checked, is the other allowed answer
        assert err.status == ARG
        frames, rflag = grp.relay(ids, counts, e1, odd.clone())
    torch.cuda.synchronize()
    for j, s in enumerate(ids):
        rows = slice(j * more, (j + 1) * more)
        assert (rflag[rows].cpu().numpy() == ch.ref[s]["relay_flag"][first:first + more]).all(), s
        assert (frames[rows].cpu().numpy() == ch.ref[s]["frames"][first:first + more]).all(), s
    assert [grp.state(s) for s in range(ns)] == [(first + more, first)] * 3 + [(0, 0)]


def test_two_live_groups_with_different_lds_needs():
    """A (10,10,10,10) group (chunks of 157 KB of LDS) and a (10,3,10,3) group at L = 1000 (127 KB) take
    turns: the kernel's raised LDS limit serves both, whichever asked last."""
    big, small = chains((10, 10, 10, 10), 300, 300), chains((10, 3, 10, 3), 1000, 120)
    ga, gb = RelayStreamGroup(300, *big.cfg, 1), RelayStreamGroup(1000, *small.cfg, 1)
    ids = np.zeros(1, dtype=np.int32)
    got_a, got_b = [], []
    for lo, hi in ((0, 60), (60, 120)):
        counts = np.array([hi - lo], dtype=np.int32)
        got_a.append(ga.relay(ids, counts, big.e1[0][lo:hi], big.cw[0][lo:hi]))
        got_b.append(gb.relay(ids, counts, small.e1[0][lo:hi], small.cw[0][lo:hi]))
    torch.cuda.synchronize()
    for got, ch in ((got_a, big), (got_b, small)):
        assert (torch.cat([g[0] for g in got]).cpu().numpy() == ch.ref[0]["frames"][:120]).all()
        assert (torch.cat([g[1] for g in got]).cpu().numpy() == ch.ref[0]["relay_flag"][:120]).all()
