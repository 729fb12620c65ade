"""In-process A/B of the stream group's two ways to code Q packets of every stream:
  (a) Q rounds of encode + decode, one packet per stream and call (the one-packet kernels);
  (b) one encode_burst + one decode_burst of Q packets per stream (the burst kernels).
10 000 streams at (10,3,3), 300-byte payloads, stream s on bin_erasure from phase 36*s (bench.py's
multistream workload), Q in {1, 4, 16, 64}; and 100 streams x 1 024 packets, bursts only.  One
process, both legs on groups in the same state fed the same packets, the legs alternating, warm-up
first; per leg the median (min .. max) over the repeats of the host-inclusive time per call (an encode +
decode pair) and per packet, and a digest of all rows and lengths, which both legs must share.
  python tools/streams_burst_ab.py [repeats]"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)

torch.cuda.set_device(0)
from fec_erasure_code_unit_test_relay_amd import StreamGroup, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

L, T, B, N = 300, 10, 3, 3
WARM = 3
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
base = load_pattern("bin_erasure")[:360000].astype(np.uint8)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def stats(ts, packets, calls):
    ts = np.sort(np.array(ts))
    med, lo, hi = float(np.median(ts)), float(ts[0]), float(ts[-1])
    return {"us_per_call": med * 1e6 / calls, "ns_per_packet": med * 1e9 / packets,
            "ns_lo": lo * 1e9 / packets, "ns_hi": hi * 1e9 / packets}


def show(name, s):
    print(f"  {name}: {s['us_per_call']:9.1f} us per call   {s['ns_per_packet']:7.3f} ns per packet "
          f"(min {s['ns_lo']:.3f} .. max {s['ns_hi']:.3f})", flush=True)


def run(NS, Q, with_a):
    reps = WARM + REPEATS
    ids = np.arange(NS, dtype=np.int32)
    counts = np.full(NS, Q, dtype=np.int32)
    pay_b = fill_payload(0, NS * Q, L, 0xA11)                        # stream-major rows [NS * Q, L]
    ph = (36 * ids.astype(np.int64)) % base.size
    # erasure flags of repeat r: packets r*Q .. r*Q+Q-1 of every stream
    er = np.stack([base[(ph + t) % base.size] for t in range(reps * Q)], axis=1)  # [NS, reps * Q]
    gb = StreamGroup(L, T, B, N, NS)
    cw_b = torch.empty((NS * Q, gb.CW), dtype=torch.uint8, device="cuda")
    wl_b = torch.empty(NS * Q, dtype=torch.int32, device="cuda")
    out_b = torch.empty((NS * Q, L), dtype=torch.uint8, device="cuda")
    ol_b = torch.empty(NS * Q, dtype=torch.int32, device="cuda")
    if with_a:
        ga = StreamGroup(L, T, B, N, NS)
        pay_a = pay_b.view(NS, Q, L).permute(1, 0, 2).contiguous()   # round-major rows [Q, NS, L]
        cw_a = torch.empty((Q, NS, gb.CW), dtype=torch.uint8, device="cuda")
        wl_a = torch.empty((Q, NS), dtype=torch.int32, device="cuda")
        out_a = torch.empty((Q, NS, L), dtype=torch.uint8, device="cuda")
        ol_a = torch.empty((Q, NS), dtype=torch.int32, device="cuda")

    def leg_a(r):
        for q in range(Q):
            ga.encode(ids, pay_a[q], out=cw_a[q], out_len=wl_a[q])
            ga.decode(ids, er_a[q], cw_a[q], out=out_a[q], out_len=ol_a[q])

    def leg_b(r):
        gb.encode_burst(ids, counts, pay_b, out=cw_b, out_len=wl_b)
        gb.decode_burst(ids, counts, er_b, cw_b, out=out_b, out_len=ol_b)

    ta, tb, same = [], [], True
    for r in range(reps):
        blk = er[:, r * Q:(r + 1) * Q]
        er_b = np.ascontiguousarray(blk).reshape(-1)
        er_a = np.ascontiguousarray(blk.T)
        legs = [(leg_b, tb)] + ([(leg_a, ta)] if with_a else [])
        if r % 2:
            legs.reverse()
        for leg, ts in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg(r)
            torch.cuda.synchronize()
            if r >= WARM:
                ts.append(time.perf_counter() - t0)
        if with_a:  # both legs coded the same packets from the same state
            same = same and torch.equal(cw_a.permute(1, 0, 2), cw_b.view(NS, Q, -1)) \
                and torch.equal(wl_a.t(), wl_b.view(NS, Q)) \
                and torch.equal(out_a.permute(1, 0, 2), out_b.view(NS, Q, L)) \
                and torch.equal(ol_a.t(), ol_b.view(NS, Q))
    print(f"{NS} streams x Q = {Q} packets per stream ({REPEATS} repeats after {WARM}):", flush=True)
    sb = stats(tb, NS * Q, 1)
    d_b = digest(cw_b, wl_b, out_b, ol_b)
    if with_a:
        sa = stats(ta, NS * Q, Q)
        d_a = digest(cw_a.permute(1, 0, 2), wl_a.t(), out_a.permute(1, 0, 2), ol_a.t())
        show("(a) one-packet calls", sa)
        show("(b) burst calls     ", sb)
        gain = sa["ns_per_packet"] - sb["ns_per_packet"]
        spread = max(sa["ns_hi"] - sa["ns_lo"], sb["ns_hi"] - sb["ns_lo"])
        print(f"  (a) - (b) = {gain:.3f} ns per packet, spread between repeats {spread:.3f}: "
              f"{'burst faster' if gain > spread else 'one-packet faster' if -gain > spread else 'no difference'}; "
              f"outputs {'identical' if same and d_a == d_b else 'DIFFER'} (digest {d_a} / {d_b})", flush=True)
        return same and d_a == d_b
    show("(b) burst calls     ", sb)
    print(f"  digest {d_b}", flush=True)
    return True


ok = True
for Q in (1, 4, 16, 64):
    ok = run(10000, Q, True) and ok
ok = run(100, 1024, False) and ok
print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
