"""Mixed message-wise relay groups (fec_mw_relay_streams_create_mixed / _set_code) on the GPU: flows of
different code pairs in one group and one launch, and a flow that changes pair in place.  Per flow the
rows of all calls together equal the one-code contract of the flow's own pair -- the reference of
tests/test_gpu_mw_relay_streams.py, whose helpers are used here -- whatever the cutting into one-packet
calls and bursts and whichever flows share a call; an output row is the flow's own hop-2 codeword and
zeros up to the group's stride.  Needs an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import fec_erasure_code_unit_test_relay_amd as fec  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.relay import (MessageWiseRelayGroup, mw_relay_streams_fit,  # noqa: E402
                                                        mw_relay_streams_mixed_fit)
from test_gpu_mw_relay_streams import (PAIRS, SEED, carve, cut_counts, flows, geometry, received,  # noqa: E402
                                       reference)

ARG = fec._lib.FEC_ERR_ARG
MTU_PAIRS = [((10, 3, 3), (10, 3, 3)), ((10, 5, 2), (6, 2, 2))]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    yield


class Source:
    """One flow's hop-1 side and what the relay must make of it: codewords [n, CW1], flags [n] and the
    reference rows (hop-2 codewords [n, CW2], sizes, fates)."""

    def __init__(self, cw1, pat, ref):
        self.cw1, self.pat, self.ref, self.n = cw1, pat, ref, pat.size
        self.CW1, self.CW2 = cw1.shape[1], ref[0].shape[1]


def source(fl, s):
    return Source(fl.cw1[s], fl.pats[s], fl.ref[s])


def random_calls(totals, choices, rng, start=0):
    """A cutting as drive() makes it, from packet `start` of every flow up to totals[s]: each call a random
    permuted subset of the live flows, half of the calls one-packet calls, the others with a count per flow
    from its own choices[s].  A list of (ids, counts, one-packet call, first seq per id)."""
    totals = np.asarray(totals, dtype=np.int64)
    sent = np.full(totals.size, start, dtype=np.int64)
    calls = []
    while (sent < totals).any():
        live = np.flatnonzero(sent < totals)
        ids = rng.permutation(live)[:max(1, int(rng.integers(1, live.size + 1)))].astype(np.int32)
        single = bool(rng.random() < 0.5)
        counts = np.array([1 if single else min(int(rng.choice(choices[s])), totals[s] - sent[s]) for s in ids],
                          dtype=np.int32)
        calls.append((ids, counts, single, sent[ids].copy()))
        sent[ids] += counts
    return calls


def padded_rows(grp, srcs, ids, counts, starts, width):
    """The call's hop-1 rows, `width` bytes each: the flow's own codeword, 0x5A behind it, and the row of an
    erased packet overwritten (never read).  Returns (rows, flags)."""
    er = np.concatenate([srcs[s].pat[a:a + c] for s, c, a in zip(ids, counts, starts)])
    parts = []
    for s, c, a in zip(ids, counts, starts):
        rows = torch.full((int(c), width), 0x5A, dtype=torch.uint8, device="cuda")
        rows[:, :srcs[s].CW1] = srcs[s].cw1[a:a + c]
        parts.append(rows)
    return received(torch.cat(parts), er), er


def relay_call(grp, srcs, ids, counts, single, starts):
    """One call: input rows padded to cw1_bytes + 3, output buffers full of 0xA5 before it."""
    rows, er = padded_rows(grp, srcs, ids, counts, starts, grp.cw1_bytes + 3)
    R = rows.shape[0]
    out = torch.full((R, grp.cw2_bytes), 0xA5, dtype=torch.uint8, device="cuda")
    wl = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    ft = torch.full((R,), 0xA5, dtype=torch.uint8, device="cuda")
    return grp.relay(ids, None if single else counts, er, rows, out=out, out_len=wl, fate=ft)


def run_calls(grp, srcs, calls, got=None, keep=None):
    """Feeds the calls; got[s] = the flow's rows of all calls together (codewords at the group's stride,
    sizes, fates), filled in place; keep: a list that takes every call's own output tensors."""
    if got is None:
        got = {s: (torch.full((src.n, grp.cw2_bytes), 0x77, dtype=torch.uint8, device="cuda"),
                   torch.full((src.n,), -7, dtype=torch.int32, device="cuda"),
                   torch.full((src.n,), 9, dtype=torch.uint8, device="cuda")) for s, src in srcs.items()}
    for ids, counts, single, starts in calls:
        res = relay_call(grp, srcs, ids, counts, single, starts)
        if keep is not None:
            keep.append(res)
        row = 0
        for s, c, a in zip(ids, counts, starts):
            for g, x in zip(got[int(s)], res):
                g[a:a + c] = x[row:row + c]
            row += c
    torch.cuda.synchronize()
    return got


def assert_rows(got, src, lo=0, hi=None, what=None):
    """Rows lo .. hi of a flow: fates, sizes and the flow's own CW2 bytes equal the reference, and the rest
    of every output row is zero."""
    hi = src.n if hi is None else hi
    cw, wl, ft = got
    r_cw, r_wl, r_ft = src.ref
    assert torch.equal(ft[lo:hi], r_ft[lo:hi]), what
    assert torch.equal(wl[lo:hi], r_wl[lo:hi]), what
    assert torch.equal(cw[lo:hi, :src.CW2], r_cw[lo:hi]), what
    assert not bool(cw[lo:hi, src.CW2:].any()), what


def pair_geometry(code, pair, src):
    (k1, n1), (k2, n2) = geometry(pair[0]), geometry(pair[1])
    return dict(code=code, k1=k1, n1=n1, k2=k2, n2=n2, cw1_bytes=src.CW1, cw2_bytes=src.CW2, delay=pair[0][0])


@pytest.mark.parametrize("L", [300, 37])
def test_five_pairs_in_one_group(L):
    """25 flows, five of each pair, 450 (+T1) packets each, in one group under random cutting: every
    flow's rows equal its own pair's reference."""
    srcs, code_of, choices = {}, [], []
    for p, pair in enumerate(PAIRS):
        fl = flows(L, *pair)
        for s in range(5):
            srcs[5 * p + s] = source(fl, s)
            code_of.append(p)
            choices.append(cut_counts(*pair))
    grp = MessageWiseRelayGroup.mixed(L, PAIRS, code_of)
    assert grp.cw1_bytes == max(s.CW1 for s in srcs.values()) and grp.cw2_bytes == max(s.CW2 for s in srcs.values())
    assert grp.delay is None and grp.code1 is None and grp.code2 is None
    assert grp.codes == [tuple(p) for p in PAIRS] and grp.code_of == code_of
    assert fec.lib().fec_mw_relay_streams_geometry(grp._h, None, None, None) == ARG
    calls = random_calls([srcs[s].n for s in range(25)], choices, np.random.default_rng(83))
    got = run_calls(grp, srcs, calls)
    for s in range(25):
        pair = PAIRS[code_of[s]]
        assert_rows(got[s], srcs[s], what=s)
        assert srcs[s].n == 450 + pair[0][0] and grp.state(s) == (450 + pair[0][0], 450), s
        assert grp.geometry(s) == pair_geometry(code_of[s], pair, srcs[s]), s


def test_one_pair_through_the_mixed_kernel_equals_the_one_code_group():
    """The same calls into a mixed group of one pair and into a plain group: every output tensor of every
    call is equal, and both equal the reference."""
    L, pair = 300, PAIRS[0]
    fl = flows(L, *pair)
    srcs = {s: source(fl, s) for s in range(fl.ns)}
    calls = random_calls([fl.total] * fl.ns, [cut_counts(*pair)] * fl.ns, np.random.default_rng(89))
    assert sum(1 for c in calls if c[2]) >= 8 and sum(1 for c in calls if not c[2] and c[1].max() > 1) >= 8
    mixed = MessageWiseRelayGroup.mixed(L, [pair], [0] * fl.ns)
    plain = MessageWiseRelayGroup(L, *pair, fl.ns)
    for name in ("cw1_bytes", "cw2_bytes", "delay", "codes", "code_of", "code1", "code2"):
        assert getattr(mixed, name) == getattr(plain, name), name
    keep_m, keep_p = [], []
    got_m = run_calls(mixed, srcs, calls, keep=keep_m)
    got_p = run_calls(plain, srcs, calls, keep=keep_p)
    assert len(keep_m) == len(keep_p) == len(calls)
    for i, (a, b) in enumerate(zip(keep_m, keep_p)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), i
    for s in range(fl.ns):
        assert_rows(got_m[s], srcs[s], what=s)
        assert_rows(got_p[s], srcs[s], what=s)
        assert mixed.state(s) == plain.state(s) == (fl.total, fl.total - pair[0][0])


LIFE = 130  # hop-1 packets of a life: more than the codeword ring's 64 rows


def life_source(L, pair, life):
    """A fresh chain of LIFE packets with its own payloads, lengths and pattern: seqs 0 and 1 erased, one
    run of B1 and one of T1+N1+2 erasures, placed as synthetic_pattern places them (at 20 and at half)."""
    (T1, B1, N1), _ = pair
    pat = np.zeros(LIFE, dtype=np.uint8)
    pat[[0, 1]] = 1
    pat[20:20 + B1] = 1
    pat[LIFE // 2:LIFE // 2 + T1 + N1 + 2] = 1
    fates = fec.plan_host(L, T1, B1, N1, pat)
    assert (fates == 2).any() and (fates == 3).any(), pair
    assert fates[0] in (2, 3) and fates[1] in (2, 3), pair  # never copied: their packets are missing
    lens = np.random.default_rng(97 + life).integers(0, L + 1, LIFE).astype(np.int32)
    lens[[5, 50]] = [0, L]
    cw1, *ref = reference(L, *pair, fec.fill_payload(0, LIFE, L, SEED + 100 + life), torch.from_numpy(lens).cuda(), pat)
    return Source(cw1, pat, ref)


def test_flow_changes_pair_in_place():
    """Flow 0 lives four lives of 130 packets on four pairs (larger and smaller CW1, T1+k1-1 and n2-1 in
    both directions) in one slot whose bytes are never cleared, beside two flows that run on: every life
    equals a fresh chain from seq 0."""
    L = 300
    order = [3, 0, 2, 1]  # (4,4,4)->(10,3,3), (10,3,3)->(10,3,3), (3,2,2)->(10,1,1), (10,5,2)->(6,2,2)
    lives = [life_source(L, PAIRS[p], i) for i, p in enumerate(order)]
    steady = {1: source(flows(L, *PAIRS[1]), 0), 2: source(flows(L, *PAIRS[4]), 0)}
    grp = MessageWiseRelayGroup.mixed(L, PAIRS, [order[0], 1, 4])
    got = run_calls(grp, steady, [])
    fed = {1: 0, 2: 0}
    sizes = [1, 1, 1, 17, 1, 40, 1, 2, 33, 1, 1, 31]  # one-packet calls and bursts; 130 in all
    assert sum(sizes) == LIFE

    def snapshot():
        return [(grp.state(s), grp.geometry(s)) for s in range(3)]

    for i, p in enumerate(order):
        if i:
            grp.set_code(0, p)
        assert grp.state(0) == (0, 0) and grp.geometry(0)["code"] == p and grp.code_of[0] == p
        assert grp.geometry(0) == pair_geometry(p, PAIRS[p], lives[i])
        srcs = {0: lives[i], **steady}
        got0, a = run_calls(grp, {0: lives[i]}, []), 0
        for j, c in enumerate(sizes):  # a call never crosses the life's end
            ids = [0] + [s for s in (1, 2) if fed[s] < steady[s].n]
            counts = np.array([c] + [min(c, steady[s].n - fed[s]) for s in ids[1:]], dtype=np.int32)
            starts = np.array([a] + [fed[s] for s in ids[1:]], dtype=np.int64)
            ids = np.array(ids, dtype=np.int32)
            call = [(ids, counts, c == 1, starts)]
            run_calls(grp, srcs, call, got={0: got0[0], **got})
            a += c
            for s, n in zip(ids[1:], counts[1:]):
                fed[int(s)] += int(n)
            if i == 2 and j == 5:  # mid-run: refused changes leave everything as it is
                before = snapshot()
                for bad in [(0, 5), (0, -1), (3, 0)]:
                    with pytest.raises(fec.FecError) as e:
                        grp.set_code(*bad)
                    assert e.value.status == ARG
                    assert snapshot() == before and grp.code_of == [p, 1, 4]
        assert_rows(got0[0], lives[i], what=("life", i))
        assert grp.state(0) == (LIFE, LIFE - PAIRS[p][0][0])
    for s in (1, 2):
        assert fed[s] == steady[s].n
        assert_rows(got[s], steady[s], what=s)


def test_set_code_on_a_one_code_group():
    """A plain group takes code 0 only, and that resets the flow: flow 0's next 100 packets, fed by one-packet
    calls, are a fresh chain; flow 1 runs on across the reset."""
    L, pair = 300, PAIRS[0]
    fl = flows(L, *pair)
    grp = MessageWiseRelayGroup(L, *pair, 2)
    srcs = {0: source(fl, 0), 1: source(fl, 1)}
    ids = np.array([0, 1], dtype=np.int32)
    calls, a = [], 0
    for c in (1, 50, 1, 68):
        calls.append((ids, np.full(2, c, dtype=np.int32), c == 1, np.full(2, a, dtype=np.int64)))
        a += c
    got = run_calls(grp, srcs, calls)
    assert grp.state(0) == grp.state(1) == (120, 110)
    with pytest.raises(fec.FecError) as e:
        grp.set_code(0, 1)
    assert e.value.status == ARG and grp.state(0) == (120, 110)
    grp.set_code(0, 0)
    assert grp.state(0) == (0, 0) and grp.state(1) == (120, 110) and grp.code_of == [0, 0]
    fresh = source(fl, 4)  # another flow's packets from its seq 0 on
    assert bool((fresh.ref[2][:100] == 2).any())
    srcs2 = {0: fresh, 1: srcs[1]}
    got2 = run_calls(grp, {0: fresh}, [])
    calls = [(ids, np.ones(2, dtype=np.int32), True, np.array([t, 120 + t], dtype=np.int64)) for t in range(100)]
    run_calls(grp, srcs2, calls, got={0: got2[0], 1: got[1]})
    assert_rows(got[0], srcs[0], hi=120)
    assert_rows(got2[0], fresh, hi=100)
    assert_rows(got[1], srcs[1], hi=220)
    assert grp.state(0) == (100, 90) and grp.state(1) == (220, 210)


def test_mtu_payloads_chunks_of_two_sizes_in_one_launch():
    """L = 1500, two pairs whose chunks hold different numbers of packets, bursts longer than either: chunks
    of two sizes in one launch, whose LDS follows the pairs present in the call."""
    L, n, code_of = 1500, 131, [0, 1, 0, 1]
    tps, lds = mw_relay_streams_mixed_fit(L, MTU_PAIRS)
    assert tps[0] != tps[1] and (lds > 64 * 1024).all()
    cuts = {0: [37, 41, n - 79, 1], 1: [41, n - 42, 1]}
    rng = np.random.default_rng(101)
    srcs = {}
    for s, c in enumerate(code_of):
        (T1, B1, N1), tp = MTU_PAIRS[c][0], int(tps[c])
        assert n - 1 > 3 * tp
        pat = np.zeros(n, dtype=np.uint8)
        pat[tp - 14 + s:tp - 14 + s + B1] = 1                # recovered, output around row tp
        pat[2 * tp - 20 + s:2 * tp - 20 + s + T1 + N1 + 2] = 1  # lost, output around row 2 tp
        fates = fec.plan_burst_host(L, T1, B1, N1, pat, np.array(cuts[c], dtype=np.int32))
        assert (fates == 2).any() and (fates == 3).any(), s
        lens = rng.integers(0, L + 1, n).astype(np.int32)
        lens[[3, 40]] = [0, L]
        cw1, *ref = reference(L, *MTU_PAIRS[c], fec.fill_payload(0, n, L, SEED + 120 + s),
                              torch.from_numpy(lens).cuda(), pat)
        srcs[s] = Source(cw1, pat, ref)
    grp = MessageWiseRelayGroup.mixed(L, MTU_PAIRS, code_of)
    even, every = np.array([0, 2], dtype=np.int32), np.array([3, 0, 1, 2], dtype=np.int32)
    at = lambda ids, a0, a1: np.array([a0 if code_of[s] == 0 else a1 for s in ids], dtype=np.int64)  # noqa: E731
    calls = [(even, np.full(2, 37, dtype=np.int32), False, at(even, 0, 0)),
             (every, np.full(4, 41, dtype=np.int32), False, at(every, 37, 0)),
             (every, (n - 1 - at(every, 78, 41)).astype(np.int32), False, at(every, 78, 41)),
             (every, np.ones(4, dtype=np.int32), True, at(every, n - 1, n - 1))]
    got = run_calls(grp, srcs, calls)
    for s in range(4):
        assert_rows(got[s], srcs[s], what=s)
        assert grp.state(s) == (n, n - 10)


@pytest.mark.parametrize("L", [300, 37])
def test_unaligned_buffers_and_strides(L):
    """A flow of each of three pairs in every call; input rows at byte offset 1 with a stride of cw1_bytes + 3,
    output rows at byte offset 1, fates at byte offset 3: rows narrower than the stride at every byte phase,
    and nothing outside the buffers is written."""
    pairs = PAIRS[:3]
    srcs = {p: source(flows(L, *pairs[p]), 4 - p) for p in range(3)}
    grp = MessageWiseRelayGroup.mixed(L, pairs, [0, 1, 2])
    W, CW2 = grp.cw1_bytes + 3, grp.cw2_bytes
    ids = np.array([2, 0, 1], dtype=np.int32)
    for a, b in zip([0, 1, 98, 162], [1, 98, 162, None]):
        counts = np.array([(srcs[s].n if b is None else b) - a for s in ids], dtype=np.int32)
        starts = np.full(3, a, dtype=np.int64)
        rx, er = padded_rows(grp, srcs, ids, counts, starts, W)
        R = rx.shape[0]
        buf, _ = carve(R * W, 1, 0xA5)
        rows = buf.as_strided((R, grp.cw1_bytes), (W, 1), buf.storage_offset())
        buf.view(R, W).copy_(rx)
        assert rows.data_ptr() % 4 == 1 and rows.stride(0) == W
        out, check_out = carve(R * CW2, 1, 0x5A)
        ft, check_ft = carve(R, 3, 0x5A)
        assert out.data_ptr() % 4 == 1 and ft.data_ptr() % 4 == 3
        wl = torch.full((R,), -1, dtype=torch.int32, device="cuda")
        grp.relay(ids, counts, er, rows, out=out.view(R, CW2), out_len=wl, fate=ft)
        torch.cuda.synchronize()
        check_out()
        check_ft()
        row = 0
        for s, c in zip(ids, counts):
            sl = slice(row, row + c)
            src = Source(srcs[s].cw1[a:a + c], srcs[s].pat[a:a + c], [r[a:a + c] for r in srcs[s].ref])
            assert_rows((out.view(R, CW2)[sl], wl[sl], ft[sl]), src, what=(int(s), a))
            row += c
    assert [grp.state(s) for s in range(3)] == [(srcs[s].n, 450) for s in range(3)]


def test_bad_arguments_leave_the_group_unchanged():
    """A flow of each pair fed 50 packets; refused calls leave every flow's state as it is, refused creates
    leave no handle, and the next valid calls continue every flow to the reference."""
    L, ns = 300, len(PAIRS)
    srcs = {p: source(flows(L, *PAIRS[p]), 0) for p in range(ns)}
    choices = [cut_counts(*p) for p in PAIRS]
    head = random_calls([50] * ns, choices, np.random.default_rng(107))
    tail = random_calls([srcs[s].n for s in range(ns)], choices, np.random.default_rng(103), start=50)
    grp = MessageWiseRelayGroup.mixed(L, PAIRS, list(range(ns)))
    got = run_calls(grp, srcs, head)
    before = [grp.state(s) for s in range(ns)]
    assert before == [(50, 50 - PAIRS[s][0][0]) for s in range(ns)]
    W = grp.cw1_bytes
    small = [s for s in range(ns) if srcs[s].CW1 < W - 1]
    assert len(small) >= 2
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    bad = [(i32(2, 2), i32(3, 3), W),                    # a repeated id
           (i32(1, ns), i32(3, 3), W),                   # an id out of range
           (i32(1, -1), i32(3, 3), W),
           (i32(1, 2), i32(6, 0), W),                    # a count of 0
           (i32(*range(ns + 1)), None, W),               # M > nstreams
           (i32(*small[:2]), i32(3, 3), W - 1)]          # cw1_stride under the group's, over the flows' own sizes
    for b_ids, b_counts, width in bad:
        R = b_ids.size if b_counts is None else 6
        rows = torch.zeros((R, width), dtype=torch.uint8, device="cuda")
        with pytest.raises(fec.FecError) as e:
            grp.relay(b_ids, b_counts, np.zeros(R, dtype=np.uint8), rows)
        assert e.value.status == ARG
        assert [grp.state(s) for s in range(ns)] == before
    # create: nothing is made
    for pairs, code_of, size in [(PAIRS, [0, ns], L), ([], [0], L), (PAIRS, None, L), (None, [0], L),
                                 (PAIRS[:4], [0, 1, 2, 3], 1500)]:
        with pytest.raises(fec.FecError) as e:
            MessageWiseRelayGroup.mixed(size, pairs, code_of)
        assert e.value.status == ARG
    assert mw_relay_streams_mixed_fit(L, PAIRS[:4])[0].size == 4  # fits at L = 300 ...
    with pytest.raises(fec.FecError):
        mw_relay_streams_fit(1500, *PAIRS[3])                     # ... (4,4,4)->(10,3,3) does not at 1500
    pr = np.array(PAIRS, dtype=np.int32).reshape(-1, 6)
    cof = np.zeros(2, dtype=np.int32)
    create = fec.lib().fec_mw_relay_streams_create_mixed
    for a_pairs, a_cof, n_codes in [(None, cof.ctypes.data, ns), (pr.ctypes.data, None, ns), (pr.ctypes.data, cof.ctypes.data, 0),
                                    (pr.ctypes.data, cof.ctypes.data, 65)]:
        h = ctypes.c_void_p()
        assert create(L, a_pairs, n_codes, a_cof, 2, ctypes.byref(h)) == ARG and h.value is None
    assert create(L, pr.ctypes.data, ns, cof.ctypes.data, 2, None) == ARG
    bad_cof = np.array([0, ns], dtype=np.int32)
    h = ctypes.c_void_p()
    assert create(L, pr.ctypes.data, ns, bad_cof.ctypes.data, 2, ctypes.byref(h)) == ARG and h.value is None
    # the next valid call continues every flow
    run_calls(grp, srcs, tail, got=got)
    for s in range(ns):
        assert_rows(got[s], srcs[s], what=s)
        assert grp.state(s) == (srcs[s].n, 450)
