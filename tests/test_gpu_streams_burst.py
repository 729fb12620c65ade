"""Stream-group bursts (fec_streams_encode_burst / fec_streams_decode_burst) on the GPU: a call that
hands over counts[m] consecutive packets of each stream equals that many one-packet calls, so every
stream's codewords, sizes, payload rows and lengths equal the oracle-checked Codec.encode /
Codec.decode over that stream alone (and, for (10,3,3), the oracle's own FEC_Encoder / FEC_Decoder
run).  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import oracle
from conftest import load_pattern

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402

SEED = 0x5EED
P = 450


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


def synthetic_pattern(T, B, N, shift):
    """P + T flags: runs of B erasures starting at 20, 60, 100, ... while the start is below P - 60,
    plus one run of T + N + 2 erasures at P / 2, all moved `shift` packets later."""
    pat = np.zeros(P + T + shift, dtype=np.uint8)
    start = 20
    while start < P - 60:
        pat[shift + start:shift + start + B] = 1
        start += 40
    pat[shift + P // 2:shift + P // 2 + T + N + 2] = 1
    return pat[:P + T]


def burst_counts(T, B, N):
    """History partly in the ring and partly in the burst, bursts longer than the 64-row ring."""
    k = T - N + 1
    n = k + B
    c = {1, 2, n - 2, n - 1, n, T + k - 1, T + k, 64 - T - k + 1, 64 - T - k + 2, 63, 64, 65, 150}
    return sorted(v for v in c if v >= 1)


class Streams:
    """ns streams of one (T,B,N): payloads, lengths, erasure patterns and the per-stream reference."""

    def __init__(self, L, tbn, ns, rng, full_first=False):
        T, B, N = tbn
        self.L, self.tbn, self.ns, self.total = L, tbn, ns, P + T
        base = load_pattern("bin_erasure").astype(np.uint8)
        self.pats = []
        for s in range(ns):
            if tbn == (10, 3, 3) and s < 4:
                self.pats.append(base[7919 * s:7919 * s + P + T].copy())
            else:
                self.pats.append(synthetic_pattern(T, B, N, 7 * s))
        self.pay = [fec.fill_payload(0, P + T, L, SEED + s) for s in range(ns)]
        self.len = []
        for s in range(ns):
            ln = rng.integers(0, L + 1, P + T).astype(np.int32)
            ln[rng.integers(0, P + T, 8)] = 0
            ln[rng.integers(0, P + T, 8)] = L
            if full_first and s == 0:  # the oracle's own run sends full payloads
                ln[:] = L
            self.len.append(torch.from_numpy(ln).cuda())
        c = fec.Codec(L, T, B, N)
        self.ref = []
        for s in range(ns):
            cw, wl = c.encode(self.pay[s], self.len[s])
            o, ol = c.decode(cw, torch.from_numpy(self.pats[s]).cuda())
            self.ref.append((cw.clone(), wl.clone(), o.clone(), ol.clone()))
        torch.cuda.synchronize()

    def assert_exercised(self):
        T, B, N = self.tbn
        fates = np.concatenate([fec.plan_host(self.L, T, B, N, p) for p in self.pats])
        assert (fates == 2).any() and (fates == 3).any()


def drive(st, grp, rng, choices, mix=False):
    """Feed every stream its P + T packets through `grp`, each call a random subset of the live
    streams with counts drawn from `choices` (mix: or a one-packet encode / decode call)."""
    T = st.tbn[0]
    ns, total, L = st.ns, st.total, st.L
    dev = st.pay[0].device
    cw = torch.zeros((ns, total, grp.CW), dtype=torch.uint8, device=dev)
    wl = torch.zeros((ns, total), dtype=torch.int32, device=dev)
    out = torch.zeros((ns, total, L), dtype=torch.uint8, device=dev)
    ol = torch.zeros((ns, total), dtype=torch.int32, device=dev)
    sent = np.zeros(ns, dtype=np.int64)
    while (sent < total).any():
        live = np.flatnonzero(sent < total)
        ids = rng.permutation(live)[:max(1, int(rng.integers(1, live.size + 1)))].astype(np.int32)
        single = mix and rng.random() < 0.5
        counts = np.array([1 if single else min(int(rng.choice(choices)), total - sent[s]) for s in ids],
                          dtype=np.int32)
        pay = torch.cat([st.pay[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
        ln = torch.cat([st.len[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
        er = np.concatenate([st.pats[s][sent[s]:sent[s] + c] for s, c in zip(ids, counts)])
        if single:
            c_cw, c_wl = grp.encode(ids, pay, ln)
        else:
            c_cw, c_wl = grp.encode_burst(ids, counts, pay, ln)
        rx = c_cw.clone()
        rx[torch.from_numpy(er.astype(bool)).to(dev)] = 0xA5  # rows of missing packets are never read
        if single:
            c_out, c_ol = grp.decode(ids, er, rx)
        else:
            c_out, c_ol = grp.decode_burst(ids, counts, er, rx)
        row = 0
        for s, c in zip(ids, counts):
            a = sent[s]
            cw[s, a:a + c], wl[s, a:a + c] = c_cw[row:row + c], c_wl[row:row + c]
            out[s, a:a + c], ol[s, a:a + c] = c_out[row:row + c], c_ol[row:row + c]
            row += c
        sent[ids] += counts
    torch.cuda.synchronize()
    for s in range(ns):
        r_cw, r_wl, r_out, r_ol = st.ref[s]
        assert torch.equal(wl[s], r_wl), s
        assert torch.equal(cw[s], r_cw), s
        assert bool((ol[s, :T] == 0).all()) and bool((out[s, :T] == 0).all()), s
        assert torch.equal(ol[s, T:], r_ol), s
        assert torch.equal(out[s, T:], r_out), s
        assert grp.state(s) == (total, total), s
    return cw, wl, out, ol


@pytest.mark.parametrize("tbn", [(10, 3, 3), (10, 5, 2), (10, 1, 1), (10, 0, 0), (3, 2, 2), (4, 4, 4)])
def test_bursts_equal_per_stream_coders(tbn):
    """13 streams of 460 packets, 300-byte payload rows of random sizes (0 and 300 among them), each
    call a random subset of the streams with burst sizes around n, T + k and the ring's 64 rows:
    every codeword, size, payload row and length equals the stream's own reference.  (10,3,3)'s
    stream 0 also equals the oracle's FEC_Encoder / FEC_Decoder run directly."""
    T, B, N = tbn
    rng = np.random.default_rng(23)
    st = Streams(300, tbn, 13, rng, full_first=tbn == (10, 3, 3))
    if B > 0:
        st.assert_exercised()
    grp = fec.StreamGroup(300, T, B, N, 13)
    cw, wl, out, ol = drive(st, grp, rng, burst_counts(T, B, N))
    if tbn == (10, 3, 3):
        ref = oracle.run_stream(300, T, B, N, P, st.pats[0], seed=SEED, want_data=True, want_codewords=True)
        assert (wl[0].cpu().numpy() == ref["cw_len"]).all()
        assert (cw[0].cpu().numpy() == ref["cw"]).all()
        assert (ol[0, T:].cpu().numpy() == ref["out_len"]).all()
        assert (out[0, T:].cpu().numpy() == ref["out_data"]).all()


def test_bursts_with_an_odd_payload_size():
    """(10,3,3) at L = 37: neither the payload rows (37 bytes) nor the codeword rows (55) are whole
    dwords, so rows start at every byte phase."""
    rng = np.random.default_rng(29)
    st = Streams(37, (10, 3, 3), 5, rng)
    st.assert_exercised()
    drive(st, fec.StreamGroup(37, 10, 3, 3, 5), rng, burst_counts(10, 3, 3))


def test_bursts_and_one_packet_calls_continue_each_other():
    rng = np.random.default_rng(31)
    st = Streams(300, (10, 3, 3), 7, rng)
    st.assert_exercised()
    drive(st, fec.StreamGroup(300, 10, 3, 3, 7), rng, burst_counts(10, 3, 3), mix=True)


def test_burst_calls_on_alternating_streams():
    """Burst calls on two HIP streams in turn, encode on one and decode on the other, ordered only
    by the caller's event on the codewords: the group orders its staging, windows and rings itself,
    so every row equals the single-stream run's."""
    T, B, N, L = 10, 3, 3, 300
    ns, total, Q = 64, 120, 8
    base = load_pattern("bin_erasure").astype(np.uint8)
    pats = np.stack([base[s * 131: s * 131 + total] for s in range(ns)])
    pays = fec.fill_payload(0, total * ns, L, SEED).view(ns, total, L)
    ids = np.arange(ns, dtype=np.int32)
    counts = np.full(ns, Q, dtype=np.int32)
    rounds = total // Q
    pay_r = [pays[:, r * Q:(r + 1) * Q].reshape(ns * Q, L).contiguous() for r in range(rounds)]
    er_r = [np.ascontiguousarray(pats[:, r * Q:(r + 1) * Q]).reshape(-1) for r in range(rounds)]

    def run(streams):
        grp = fec.StreamGroup(L, T, B, N, ns)
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
    c = fec.Codec(L, T, B, N)
    cw0, wl0 = c.encode(pays[5].contiguous())
    o0, ol0 = c.decode(cw0, torch.from_numpy(pats[5]).cuda())
    got_cw = ref[0].view(rounds, ns, Q, -1)[:, 5].reshape(total, -1)
    got_out = ref[2].view(rounds, ns, Q, L)[:, 5].reshape(total, L)
    got_ol = ref[3].view(rounds, ns, Q)[:, 5].reshape(total)
    assert torch.equal(got_cw, cw0)
    assert torch.equal(got_ol[T:], ol0) and torch.equal(got_out[T:], o0)


def test_a_call_larger_than_the_groups_staging():
    """4 streams x 5 000 packets in one encode call and one decode call (a 4-stream group's staging
    holds a few records)."""
    T, B, N, L = 10, 3, 3, 300
    ns, cnt = 4, 5000
    base = load_pattern("bin_erasure").astype(np.uint8)
    pats = [base[7919 * s:7919 * s + cnt].copy() for s in range(ns)]
    pays = [fec.fill_payload(0, cnt, L, SEED + s) for s in range(ns)]
    c = fec.Codec(L, T, B, N)
    grp = fec.StreamGroup(L, T, B, N, ns)
    ids = np.array([2, 0, 3, 1], dtype=np.int32)
    counts = np.full(ns, cnt, dtype=np.int32)
    cw, wl = grp.encode_burst(ids, counts, torch.cat([pays[s] for s in ids]))
    er = np.concatenate([pats[s] for s in ids])
    rx = cw.clone()
    rx[torch.from_numpy(er.astype(bool)).cuda()] = 0xA5
    out, ol = grp.decode_burst(ids, counts, er, rx)
    torch.cuda.synchronize()
    for j, s in enumerate(ids):
        r_cw, r_wl = c.encode(pays[s])
        r_out, r_ol = c.decode(r_cw, torch.from_numpy(pats[s]).cuda())
        rows = slice(j * cnt, (j + 1) * cnt)
        assert torch.equal(cw[rows], r_cw) and torch.equal(wl[rows], r_wl), s
        assert bool((ol[rows][:T] == 0).all()), s
        assert torch.equal(ol[rows][T:], r_ol) and torch.equal(out[rows][T:], r_out), s
        assert grp.state(int(s)) == (cnt, cnt)


def test_burst_calls_reject_bad_arguments():
    L, ns = 300, 8
    grp = fec.StreamGroup(L, 10, 3, 3, ns)
    ids = np.arange(3, dtype=np.int32)
    counts = np.array([4, 2, 3], dtype=np.int32)
    pay = fec.fill_payload(0, 9, L, SEED)
    cw, _ = grp.encode_burst(ids, counts, pay)
    grp.decode_burst(ids, counts, np.zeros(9, dtype=np.uint8), cw)
    torch.cuda.synchronize()
    before = [grp.state(s) for s in range(ns)]
    assert before[:3] == [(4, 4), (2, 2), (3, 3)]
    bad = [(np.array([3, 3], dtype=np.int32), np.array([2, 2], dtype=np.int32)),    # repeated id
           (np.array([1, 2], dtype=np.int32), np.array([4, 0], dtype=np.int32)),    # a count of 0
           (np.array([1, 2], dtype=np.int32), np.array([5, -1], dtype=np.int32)),   # a negative count
           (np.arange(ns + 1, dtype=np.int32), np.full(ns + 1, 2, dtype=np.int32))]  # M > nstreams
    for b_ids, b_counts in bad:
        R = int(np.maximum(b_counts, 0).sum())
        p = fec.fill_payload(0, R, L, SEED)
        c = torch.zeros((R, grp.CW), dtype=torch.uint8, device="cuda")
        with pytest.raises(fec.FecError):
            grp.encode_burst(b_ids, b_counts, p)
        with pytest.raises(fec.FecError):
            grp.decode_burst(b_ids, b_counts, np.zeros(R, dtype=np.uint8), c)
        assert [grp.state(s) for s in range(ns)] == before


def test_bursts_at_mtu_size_payloads():
    """(10,3,3) at L = 1500: the chunks take more than 64 KB of LDS (the kernels' raised limit)."""
    rng = np.random.default_rng(37)
    st = Streams(1500, (10, 3, 3), 3, rng)
    st.assert_exercised()
    drive(st, fec.StreamGroup(1500, 10, 3, 3, 3), rng, burst_counts(10, 3, 3))


def test_few_long_bursts_on_a_group_with_a_planner_pool(monkeypatch):
    """3 streams x 700, then x 324 packets on a 2 048-stream group whose symbolic steps run on a pool of 8
    threads: more parts than streams in the call, so some parts are empty."""
    monkeypatch.setenv("FEC_STREAMS_THREADS", "8")
    T, B, N, L = 10, 3, 3, 300
    cnt = 1024
    base = load_pattern("bin_erasure").astype(np.uint8)
    ids = np.array([2047, 5, 1000], dtype=np.int32)
    pats = [base[7919 * j:7919 * j + cnt].copy() for j in range(3)]
    pays = [fec.fill_payload(0, cnt, L, SEED + j) for j in range(3)]
    c = fec.Codec(L, T, B, N)
    grp = fec.StreamGroup(L, T, B, N, 2048)
    got = []
    for a, b in ((0, 700), (700, cnt)):
        counts = np.full(3, b - a, dtype=np.int32)
        cw, wl = grp.encode_burst(ids, counts, torch.cat([p[a:b] for p in pays]))
        er = np.concatenate([p[a:b] for p in pats])
        rx = cw.clone()
        rx[torch.from_numpy(er.astype(bool)).cuda()] = 0xA5
        out, ol = grp.decode_burst(ids, counts, er, rx)
        got.append([x.view(3, b - a, -1) for x in (cw, wl, out, ol)])
    torch.cuda.synchronize()
    cw, wl, out, ol = [torch.cat([g[i] for g in got], dim=1) for i in range(4)]
    for j, s in enumerate(ids):
        r_cw, r_wl = c.encode(pays[j])
        r_out, r_ol = c.decode(r_cw, torch.from_numpy(pats[j]).cuda())
        assert torch.equal(cw[j], r_cw) and torch.equal(wl[j, :, 0], r_wl), s
        assert bool((ol[j, :T] == 0).all()), s
        assert torch.equal(ol[j, T:, 0], r_ol) and torch.equal(out[j, T:], r_out), s
        assert grp.state(int(s)) == (cnt, cnt)
    assert grp.state(0) == (0, 0)


def test_burst_calls_refuse_a_geometry_beyond_the_lds():
    """(24,12,12) at L = 1500 (k = 13, n = 25): a chunk with the 24 windows / 36 codewords in front
    of it does not fit a CU's 160 KB of LDS: both calls return FEC_ERR_ARG and leave the group as it
    was."""
    L, ns = 1500, 4
    grp = fec.StreamGroup(L, 24, 12, 12, ns)
    ids = np.array([0, 2], dtype=np.int32)
    counts = np.array([2, 3], dtype=np.int32)
    pay = torch.zeros((5, L), dtype=torch.uint8, device="cuda")
    cw = torch.zeros((5, grp.CW), dtype=torch.uint8, device="cuda")
    with pytest.raises(fec.FecError) as e:
        grp.encode_burst(ids, counts, pay)
    assert e.value.status == fec._lib.FEC_ERR_ARG
    with pytest.raises(fec.FecError) as e:
        grp.decode_burst(ids, counts, np.zeros(5, dtype=np.uint8), cw)
    assert e.value.status == fec._lib.FEC_ERR_ARG
    assert [grp.state(s) for s in range(ns)] == [(0, 0)] * ns
