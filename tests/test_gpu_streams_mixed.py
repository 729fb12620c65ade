"""Mixed stream groups (fec_streams_create_mixed) on the GPU: streams of different (T,B,N) in one
group, coded together in one launch per call and direction.  Per stream, all its rows over all calls
equal the oracle-checked Codec.encode / Codec.decode of its own (T,B,N) over its whole sequence,
whatever the cutting into one-packet calls and bursts and whichever streams shared its calls (and,
for a (10,3,3) stream, the oracle's own FEC_Encoder / FEC_Decoder run).  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import oracle
from conftest import load_pattern

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402

SEED = 0x5EED
P = 450
TOTAL = 460
SIX = [(10, 3, 3), (10, 5, 2), (10, 1, 1), (10, 0, 0), (3, 2, 2), (4, 4, 4)]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def synthetic_pattern(T, B, N, shift, total=TOTAL):
    """`total` flags: runs of B erasures starting at 20, 60, 100, ... while the start is below P - 60,
    plus one run of T + N + 2 erasures at P / 2, all moved `shift` packets later."""
    pat = np.zeros(max(total, P + T) + shift, dtype=np.uint8)
    start = 20
    while start < P - 60:
        pat[shift + start:shift + start + B] = 1
        start += 40
    pat[shift + P // 2:shift + P // 2 + T + N + 2] = 1
    return pat[:total]


def burst_counts(T, B, N):
    """History partly in the ring and partly in the burst, bursts longer than the 64-row ring."""
    k = T - N + 1
    n = k + B
    c = {1, 2, n - 2, n - 1, n, T + k - 1, T + k, 64 - T - k + 1, 64 - T - k + 2, 63, 64, 65, 150}
    return sorted(v for v in c if v >= 1)


_codecs = {}


def codec(L, tbn):
    if (L, tbn) not in _codecs:
        _codecs[(L, tbn)] = fec.Codec(L, *tbn)
    return _codecs[(L, tbn)]


class Streams:
    """Streams of `total` packets each, stream s of code tuples[code_of[s]]: payloads, lengths,
    erasure patterns (the code's own synthetic pattern; bin/erasure.bin's first flags and full
    payloads for stream 0 when full_first) and the per-stream reference, computed once."""

    def __init__(self, L, tuples, code_of, rng, total=TOTAL, full_first=False):
        self.L, self.tuples, self.code_of, self.ns, self.total = L, tuples, list(code_of), len(code_of), total
        self.pats, self.pay, self.len, self.ref = [], [], [], []
        for s, c in enumerate(self.code_of):
            T, B, N = tuples[c]
            if full_first and s == 0:
                self.pats.append(load_pattern("bin_erasure").astype(np.uint8)[:total].copy())
            else:
                self.pats.append(synthetic_pattern(T, B, N, 7 * s, total))
            self.pay.append(fec.fill_payload(0, total, L, SEED + s))
            ln = rng.integers(0, L + 1, total).astype(np.int32)
            ln[rng.integers(0, total, 8)] = 0
            ln[rng.integers(0, total, 8)] = L
            if full_first and s == 0:  # the oracle's own run sends full payloads
                ln[:] = L
            self.len.append(torch.from_numpy(ln).cuda())
            self.ref.append(self.reference(s, tuples[c], 0, total))
        torch.cuda.synchronize()

    def reference(self, s, tbn, a, b):
        """(codewords, sizes, payload rows, lengths) of a fresh coder of `tbn` over packets a .. b-1 of stream s."""
        c = codec(self.L, tbn)
        cw, wl = c.encode(self.pay[s][a:b].contiguous(), self.len[s][a:b].contiguous())
        o, ol = c.decode(cw, torch.from_numpy(self.pats[s][a:b]).cuda())
        return cw.clone(), wl.clone(), o.clone(), ol.clone()

    def assert_exercised(self):
        """Every code with B > 0: its streams' patterns produce both recovered and lost packets."""
        for c, (T, B, N) in enumerate(self.tuples):
            mine = [s for s in range(self.ns) if self.code_of[s] == c]
            if B == 0 or not mine:
                continue
            fates = np.concatenate([fec.plan_host(self.L, T, B, N, self.pats[s]) for s in mine])
            assert (fates == 2).any() and (fates == 3).any(), (T, B, N)


class Rows:
    """What the calls gave, per stream and packet."""

    def __init__(self, st, CW):
        dev = st.pay[0].device
        self.cw = torch.zeros((st.ns, st.total, CW), dtype=torch.uint8, device=dev)
        self.wl = torch.zeros((st.ns, st.total), dtype=torch.int32, device=dev)
        self.out = torch.zeros((st.ns, st.total, st.L), dtype=torch.uint8, device=dev)
        self.ol = torch.zeros((st.ns, st.total), dtype=torch.int32, device=dev)


def one_call(st, grp, res, ids, counts, sent, single):
    """Packets sent[s] .. sent[s] + counts - 1 of every stream of ids through one encode and one decode call."""
    dev = st.pay[0].device
    pay = torch.cat([st.pay[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
    ln = torch.cat([st.len[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
    er = np.concatenate([st.pats[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
    if single:
        c_cw, c_wl = grp.encode(ids, pay, ln)
    else:
        c_cw, c_wl = grp.encode_burst(ids, counts, pay, ln)
    rx = c_cw.clone()
    rx[torch.from_numpy(er.astype(bool)).to(dev)] = 0xA5  # rows of missing packets are never read
    for s, c, r in zip(ids, counts, np.cumsum(counts) - counts):  # nor are a row's bytes past the stream's own CW
        rx[r:r + c, grp.geometry(int(s))["CW"]:] = 0x5A
    if single:
        c_out, c_ol = grp.decode(ids, er, rx)
    else:
        c_out, c_ol = grp.decode_burst(ids, counts, er, rx)
    row = 0
    for s, c in zip(ids, counts):
        a = sent[s]
        res.cw[s, a:a + c], res.wl[s, a:a + c] = c_cw[row:row + c], c_wl[row:row + c]
        res.out[s, a:a + c], res.ol[s, a:a + c] = c_out[row:row + c], c_ol[row:row + c]
        row += c
    return c_cw, c_wl, c_out, c_ol


def drive(st, grps, rng, lo=0, hi=None, p_single=0.0):
    """Feed packets lo .. hi-1 of every stream through every group of `grps` (the same calls to each):
    each call a random subset of the live streams, every stream's count drawn from its own code's
    burst_counts (or, with probability p_single, a one-packet encode / decode call).  Returns a Rows
    per group and the per-call outputs of each."""
    hi = st.total if hi is None else hi
    res = [Rows(st, g.CW) for g in grps]
    calls = [[] for _ in grps]
    sent = np.full(st.ns, lo, dtype=np.int64)
    while (sent < hi).any():
        live = np.flatnonzero(sent < hi)
        ids = rng.permutation(live)[:max(1, int(rng.integers(1, live.size + 1)))].astype(np.int32)
        single = rng.random() < p_single
        counts = np.array([1 if single else min(int(rng.choice(burst_counts(*st.tuples[st.code_of[s]]))), hi - sent[s])
                           for s in ids], dtype=np.int32)
        for g, r, cl in zip(grps, res, calls):
            cl.append(one_call(st, g, r, ids, counts, sent, single))
        sent[ids] += counts
    torch.cuda.synchronize()
    return res, calls


def check_stream(st, grp, res, s, ref, a, b):
    """Rows a .. b-1 of stream s equal `ref`, the reference of a coder that started at packet a."""
    geo = grp.geometry(s)
    T, CW = geo["T"], geo["CW"]
    r_cw, r_wl, r_out, r_ol = ref
    assert r_cw.shape[1] == CW
    assert torch.equal(res.wl[s, a:b], r_wl), s
    assert torch.equal(res.cw[s, a:b, :CW], r_cw), s
    assert bool((res.cw[s, a:b, CW:] == 0).all()), s
    assert bool((res.ol[s, a:a + T] == 0).all()) and bool((res.out[s, a:a + T] == 0).all()), s
    assert torch.equal(res.ol[s, a + T:b], r_ol), s
    assert torch.equal(res.out[s, a + T:b], r_out), s


def check_all(st, grp, res):
    for s in range(st.ns):
        check_stream(st, grp, res, s, st.ref[s], 0, st.total)
        assert grp.state(s) == (st.total, st.total), s


def test_six_codes_in_one_group():
    """13 streams over six codes, 460 packets each, 300-byte payload rows of random sizes (0 and 300
    among them), each call a random subset of the streams with each stream's burst size around its own
    n, T + k and the ring's 64 rows: every codeword, size, payload row and length equals the stream's
    own reference, the rest of each codeword row is zero, and stream 0 also equals the oracle's
    FEC_Encoder / FEC_Decoder run directly."""
    rng = np.random.default_rng(41)
    code_of = [s % 6 for s in range(13)]
    st = Streams(300, SIX, code_of, rng, full_first=True)
    st.assert_exercised()
    grp = fec.StreamGroup.mixed(300, SIX, code_of)
    assert grp.CW == max(-(-(302) // (T - N + 1)) * (T - N + 1 + B) for T, B, N in SIX)
    assert grp.T is None and grp.k is None and grp.n is None and grp.S is None
    assert grp.codes == SIX and grp.code_of.tolist() == code_of
    (res,), _ = drive(st, [grp], rng)
    check_all(st, grp, res)
    ref = oracle.run_stream(300, 10, 3, 3, P, st.pats[0], seed=SEED, want_data=True, want_codewords=True)
    CW = grp.geometry(0)["CW"]
    assert (res.wl[0].cpu().numpy() == ref["cw_len"]).all()
    assert (res.cw[0, :, :CW].cpu().numpy() == ref["cw"]).all()
    assert (res.ol[0, 10:].cpu().numpy() == ref["out_len"]).all()
    assert (res.out[0, 10:].cpu().numpy() == ref["out_data"]).all()


@pytest.mark.parametrize("tuples", [[(10, 3, 3), (3, 2, 2), (10, 5, 2)], [(10, 3, 3), (10, 1, 1), (10, 0, 0)]])
def test_mixed_group_with_an_odd_payload_size(tuples):
    """L = 37, 6 streams: payload rows of 37 bytes, so they start at every byte phase.  With (10,3,3),
    (3,2,2) and (10,5,2) the codewords are 55, 80 and 70 bytes in rows of 80, which no longer lie at
    their LDS phase; with (10,3,3), (10,1,1) and (10,0,0) they are 55, 44 and 44 bytes in rows of 55,
    a stride that is no multiple of 4, so the codeword rows start at every byte phase too."""
    rng = np.random.default_rng(43)
    code_of = [s % 3 for s in range(6)]
    st = Streams(37, tuples, code_of, rng)
    st.assert_exercised()
    grp = fec.StreamGroup.mixed(37, tuples, code_of)
    assert grp.CW == (80 if (3, 2, 2) in tuples else 55)
    assert len({grp.geometry(s)["CW"] for s in range(6)}) >= 2
    (res,), _ = drive(st, [grp], rng)
    check_all(st, grp, res)


def test_bursts_and_one_packet_calls_continue_each_other():
    rng = np.random.default_rng(47)
    tuples = [(10, 3, 3), (10, 5, 2), (3, 2, 2)]
    code_of = [s % 3 for s in range(7)]
    st = Streams(300, tuples, code_of, rng)
    st.assert_exercised()
    grp = fec.StreamGroup.mixed(300, tuples, code_of)
    (res,), _ = drive(st, [grp], rng, p_single=0.5)
    check_all(st, grp, res)


def test_one_code_through_the_mixed_kernels_equals_the_one_code_group():
    """The same calls to StreamGroup.mixed(300, [(10,3,3)], zeros) and StreamGroup(300,10,3,3): every
    output tensor of every call is equal, row for row -- the new kernels against the old ones."""
    rng = np.random.default_rng(53)
    st = Streams(300, [(10, 3, 3)], [0] * 5, rng)
    st.assert_exercised()
    new = fec.StreamGroup.mixed(300, [(10, 3, 3)], np.zeros(5, dtype=np.int32))
    old = fec.StreamGroup(300, 10, 3, 3, 5)
    assert new.CW == old.CW == new.geometry(0)["CW"]
    (r_new, r_old), (c_new, c_old) = drive(st, [new, old], rng, p_single=0.5)
    assert len(c_new) == len(c_old) > 0
    for a, b in zip(c_new, c_old):
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y)
    check_all(st, new, r_new)


def test_set_code_starts_a_fresh_coder_in_place():
    """Stream 1 goes from (10,3,3) to (10,5,2) after 100 packets: its next 100 equal a fresh
    Codec(300,10,5,2) over those packets alone, the other streams run on uninterrupted."""
    rng = np.random.default_rng(59)
    tuples = [(10, 3, 3), (10, 5, 2)]
    st = Streams(300, tuples, [0, 0, 1, 1], rng, total=200)
    grp = fec.StreamGroup.mixed(300, tuples, st.code_of)
    (res1,), _ = drive(st, [grp], rng, 0, 100, p_single=0.5)
    assert [grp.state(s) for s in range(4)] == [(100, 100)] * 4
    with pytest.raises(fec.FecError) as e:
        grp.set_code(1, 2)
    assert e.value.status == fec._lib.FEC_ERR_ARG
    assert [grp.state(s) for s in range(4)] == [(100, 100)] * 4 and grp.geometry(1)["code"] == 0
    check_stream(st, grp, res1, 1, st.reference(1, (10, 3, 3), 0, 100), 0, 100)
    grp.set_code(1, 1)
    assert grp.state(1) == (0, 0) and grp.geometry(1)["code"] == 1 and grp.code_of.tolist() == [0, 1, 1, 1]
    st.code_of[1] = 1  # its burst sizes from now on
    (res2,), _ = drive(st, [grp], rng, 100, 200, p_single=0.5)
    check_stream(st, grp, res2, 1, st.reference(1, (10, 5, 2), 100, 200), 100, 200)
    assert grp.state(1) == (100, 100)
    for s in (0, 2, 3):
        both = Rows(st, grp.CW)
        for name in ("cw", "wl", "out", "ol"):
            getattr(both, name)[s, :100] = getattr(res1, name)[s, :100]
            getattr(both, name)[s, 100:] = getattr(res2, name)[s, 100:]
        check_stream(st, grp, both, s, st.ref[s], 0, 200)
        assert grp.state(s) == (200, 200)


def test_set_code_on_a_one_code_group_resets_the_stream():
    """A group made by fec_streams_create takes only code 0, which makes the stream a fresh coder: after
    100 packets, stream 0's next 100 through one-packet calls (its pattern erases the first three of
    them, so their recovery reaches in front of the new start) equal a fresh Codec over them alone."""
    rng = np.random.default_rng(67)
    st = Streams(300, [(10, 3, 3)], [0, 0], rng, total=200)
    assert st.pats[0][100:103].all()
    one = fec.StreamGroup(300, 10, 3, 3, 2)
    (res1,), _ = drive(st, [one], rng, 0, 100, p_single=0.5)
    with pytest.raises(fec.FecError) as e:
        one.set_code(0, 1)
    assert e.value.status == fec._lib.FEC_ERR_ARG and one.state(0) == (100, 100)
    one.set_code(0, 0)
    assert one.state(0) == (0, 0) and one.state(1) == (100, 100)
    (res2,), _ = drive(st, [one], rng, 100, 200, p_single=1.0)
    check_stream(st, one, res2, 0, st.reference(0, (10, 3, 3), 100, 200), 100, 200)
    res2.cw[1, :100], res2.wl[1, :100] = res1.cw[1, :100], res1.wl[1, :100]
    res2.out[1, :100], res2.ol[1, :100] = res1.out[1, :100], res1.ol[1, :100]
    check_stream(st, one, res2, 1, st.ref[1], 0, 200)
    assert one.state(0) == (100, 100) and one.state(1) == (200, 200)


def test_mixed_calls_on_alternating_streams():
    """Calls on two HIP streams in turn, encode on one and decode on the other, ordered only by the
    caller's event on the codewords: the group orders its staging, windows and rings itself, so every
    row equals the single-stream run's."""
    L, ns, Q, rounds = 300, 12, 8, 10
    tuples = [(10, 3, 3), (10, 5, 2)]
    code_of = [s % 2 for s in range(ns)]
    total = Q * rounds
    base = load_pattern("bin_erasure").astype(np.uint8)
    pats = np.stack([base[s * 131: s * 131 + total] for s in range(ns)])
    pays = fec.fill_payload(0, total * ns, L, SEED).view(ns, total, L)
    ids = np.arange(ns, dtype=np.int32)
    counts = np.full(ns, Q, dtype=np.int32)
    pay_r = [pays[:, r * Q:(r + 1) * Q].reshape(ns * Q, L).contiguous() for r in range(rounds)]
    er_r = [np.ascontiguousarray(pats[:, r * Q:(r + 1) * Q]).reshape(-1) for r in range(rounds)]

    def run(streams):
        grp = fec.StreamGroup.mixed(L, tuples, code_of)
        cws = torch.empty((rounds, ns * Q, grp.CW), dtype=torch.uint8, device="cuda")
        wls = torch.empty((rounds, ns * Q), dtype=torch.int32, device="cuda")
        outs = torch.zeros((rounds, ns * Q, L), dtype=torch.uint8, device="cuda")
        ols = torch.zeros((rounds, ns * Q), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for r in range(rounds):
            se, sd = streams[r % len(streams)], streams[(r + 1) % len(streams)]
            with torch.cuda.stream(se):
                grp.encode_burst(ids, counts, pay_r[r], out=cws[r], out_len=wls[r])
                ev = torch.cuda.Event()
                ev.record()
            with torch.cuda.stream(sd):
                sd.wait_event(ev)  # the caller's own dependency: codewords of this round
                grp.decode_burst(ids, counts, er_r[r], cws[r], out=outs[r], out_len=ols[r])
        torch.cuda.synchronize()
        return cws, wls, outs, ols

    ref = run([torch.cuda.current_stream()])
    got = run([torch.cuda.Stream(), torch.cuda.Stream()])
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    # and the single-stream run is the per-stream coders'
    for s in (4, 5):
        T, B, N = tuples[code_of[s]]
        c = codec(L, tuples[code_of[s]])
        cw0, wl0 = c.encode(pays[s].contiguous())
        o0, ol0 = c.decode(cw0, torch.from_numpy(pats[s]).cuda())
        got_cw = ref[0].view(rounds, ns, Q, -1)[:, s].reshape(total, -1)
        got_out = ref[2].view(rounds, ns, Q, L)[:, s].reshape(total, L)
        got_ol = ref[3].view(rounds, ns, Q)[:, s].reshape(total)
        assert torch.equal(got_cw[:, :cw0.shape[1]], cw0) and bool((got_cw[:, cw0.shape[1]:] == 0).all())
        assert torch.equal(got_ol[T:], ol0) and torch.equal(got_out[T:], o0)


def test_mixed_group_at_mtu_size_payloads():
    """L = 1500, (10,3,3) and (10,5,2): the chunks take more than 64 KB of LDS, (10,5,2)'s more than
    (10,3,3)'s.  A call holding only the (10,3,3) streams comes first, then one holding both: the
    launch's LDS follows the codes present in the call."""
    rng = np.random.default_rng(61)
    tuples = [(10, 3, 3), (10, 5, 2)]
    code_of = [0, 1, 0, 1]
    st = Streams(1500, tuples, code_of, rng, total=200)
    ec, el, dc, dl = fec.streams_mixed_fit(1500, tuples)
    assert 65536 < el[0] < el[1] and 65536 < dl[0] < dl[1]
    grp = fec.StreamGroup.mixed(1500, tuples, code_of)
    res = Rows(st, grp.CW)
    sent = np.zeros(4, dtype=np.int64)
    for ids, cnt in (([0, 2], 37), ([3, 0, 1, 2], 41)):
        ids = np.array(ids, dtype=np.int32)
        counts = np.full(ids.size, cnt, dtype=np.int32)
        one_call(st, grp, res, ids, counts, sent, False)
        sent[ids] += counts
    while (sent < st.total).any():
        ids = rng.permutation(np.flatnonzero(sent < st.total)).astype(np.int32)
        counts = np.array([min(int(rng.choice(burst_counts(*tuples[code_of[s]]))), st.total - sent[s]) for s in ids],
                          dtype=np.int32)
        one_call(st, grp, res, ids, counts, sent, False)
        sent[ids] += counts
    torch.cuda.synchronize()
    check_all(st, grp, res)


def test_mixed_groups_reject_bad_arguments():
    L = 300
    tuples = [(10, 3, 3), (10, 5, 2)]
    for tup, cof, pay in ((tuples, [0, 2, 1], L),                       # a code index equal to ncodes
                          (np.zeros((0, 3), dtype=np.int32), [0], L),    # no codes
                          (tuples + [(24, 12, 12)], [0, 1, 2], 1500)):  # a code whose chunks do not fit
        with pytest.raises(fec.FecError) as e:
            fec.StreamGroup.mixed(pay, tup, cof)
        assert e.value.status == fec._lib.FEC_ERR_ARG
    ns = 8
    grp = fec.StreamGroup.mixed(L, tuples, [s % 2 for s in range(ns)])
    ids = np.arange(3, dtype=np.int32)
    counts = np.array([4, 2, 3], dtype=np.int32)
    cw, _ = grp.encode_burst(ids, counts, fec.fill_payload(0, 9, L, SEED))
    grp.decode_burst(ids, counts, np.zeros(9, dtype=np.uint8), cw)
    torch.cuda.synchronize()
    before = [grp.state(s) for s in range(ns)]
    assert before[:3] == [(4, 4), (2, 2), (3, 3)]
    bad = [(np.array([3, 3], dtype=np.int32), np.array([2, 2], dtype=np.int32)),    # repeated id
           (np.array([1, 2], dtype=np.int32), np.array([4, 0], dtype=np.int32)),    # a count of 0
           (np.arange(ns + 1, dtype=np.int32), np.full(ns + 1, 2, dtype=np.int32))]  # M > nstreams
    for b_ids, b_counts in bad:
        R = int(np.maximum(b_counts, 0).sum())
        p = fec.fill_payload(0, R, L, SEED)
        c = torch.zeros((R, grp.CW), dtype=torch.uint8, device="cuda")
        with pytest.raises(fec.FecError) as e:
            grp.encode_burst(b_ids, b_counts, p)
        assert e.value.status == fec._lib.FEC_ERR_ARG
        with pytest.raises(fec.FecError) as e:
            grp.decode_burst(b_ids, b_counts, np.zeros(R, dtype=np.uint8), c)
        assert e.value.status == fec._lib.FEC_ERR_ARG
        assert [grp.state(s) for s in range(ns)] == before
    # one-packet calls: a repeated id, M > nstreams
    for b_ids in (np.array([3, 3], dtype=np.int32), np.arange(ns + 1, dtype=np.int32)):
        M = b_ids.size
        with pytest.raises(fec.FecError):
            grp.encode(b_ids, fec.fill_payload(0, M, L, SEED))
        with pytest.raises(fec.FecError):
            grp.decode(b_ids, np.zeros(M, dtype=np.uint8), torch.zeros((M, grp.CW), dtype=torch.uint8, device="cuda"))
        assert [grp.state(s) for s in range(ns)] == before
