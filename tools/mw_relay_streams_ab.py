"""In-process A/B of the two ways a node relays many message-wise (type-1) flows, Q packets of every
flow per step:
  (a) a message-wise relay group (MessageWiseRelayGroup): one relay call, hop-1 decode and hop-2
      encode in one launch;
  (b) the composition it fuses: StreamGroup(code1).decode_burst, then StreamGroup(code2).encode_burst
      of the decoder's rows with lengths clipped to [0, L] (a clamp on the GPU, counted in the leg) --
      two launches, two host passes, every forwarded message written to memory as a payload row and
      read back.  Rows of hop-1 seq < T1 carry no message: leg (b) feeds its encoder only from seq T1
      on, which happens in warm-up steps alone.
10 000 flows of (10,3,3) -> (10,3,3), 300-byte payloads, at Q in {1, 16, 64} (Q = 1: one-packet calls),
and 100 flows x 1 024; flow s's hop 1 on bin_erasure from phase 36*s.  The hop-1 rows are real
FEC_Encoder codewords of one continuous source stream per flow (the relay's outputs depend on it).  One
process, both legs fed the same rows from the same state, the legs alternating (the order swaps every
repeat), 3 warm-up steps first (11 at Q = 1: until every flow forwards a message per packet); per leg
the median (min .. max) over the repeats of the host-inclusive time per packet, calls plus one synchronise.  After every repeat leg (b)'s codewords and sizes must equal
leg (a)'s.  --group-only runs leg (a) alone (for a kernel trace), --composition-only leg (b).
  timeout -k 10 900 python tools/mw_relay_streams_ab.py [repeats] [--group-only | --composition-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)

torch.cuda.set_device(0)
from fec_erasure_code_unit_test_relay_amd import StreamGroup, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.relay import MessageWiseRelayGroup  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

L, CODE1, CODE2 = 300, (10, 3, 3), (10, 3, 3)
WARM = 3
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPEATS = int(args[0]) if args else 9
LEGS = "a" if "--group-only" in sys.argv else "b" if "--composition-only" in sys.argv else "ab"
pat1 = load_pattern("bin_erasure")[:360000].astype(np.uint8)


def show(name, ts, packets):
    ts = np.sort(np.array(ts)) * 1e9 / packets
    print(f"  {name}: {float(np.median(ts)):9.2f} ns per packet (min {ts[0]:.2f} .. max {ts[-1]:.2f})", flush=True)
    return float(np.median(ts)), float(ts[0]), float(ts[-1])


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(NS, Q):
    T1 = CODE1[0]
    warm = max(WARM, -(-(T1 + 1) // Q))  # every timed step forwards Q messages per flow
    reps = warm + REPEATS
    assert Q == 1 or Q >= T1  # leg (b)'s first step: at most one split burst
    ids = np.arange(NS, dtype=np.int32)
    full = np.full(NS, Q, dtype=np.int32)
    counts = None if Q == 1 else full
    ph = (36 * np.arange(NS, dtype=np.int64)) % pat1.size
    src = StreamGroup(L, *CODE1, NS)
    grp = MessageWiseRelayGroup(L, CODE1, CODE2, NS)
    dec, enc = StreamGroup(L, *CODE1, NS), StreamGroup(L, *CODE2, NS)
    R = NS * Q
    cw2_a = torch.zeros((R, grp.cw2_bytes), dtype=torch.uint8, device="cuda")
    wl_a = torch.zeros(R, dtype=torch.int32, device="cuda")
    ft_a = torch.zeros(R, dtype=torch.uint8, device="cuda")
    msg = torch.zeros((R, L), dtype=torch.uint8, device="cuda")
    ml = torch.zeros(R, dtype=torch.int32, device="cuda")
    cw2_b = torch.zeros((R, grp.cw2_bytes), dtype=torch.uint8, device="cuda")
    wl_b = torch.zeros(R, dtype=torch.int32, device="cuda")
    t = {"a": [], "b": []}
    same = True
    for r in range(reps):
        cw1, _ = src.encode_burst(ids, full, fill_payload(r * R, R, L, 0xA11))
        er = np.ascontiguousarray(np.stack([pat1[(ph + r * Q + q) % pat1.size] for q in range(Q)], axis=1)).reshape(-1)
        fed = r * Q  # hop-1 packets every flow has been fed before this step

        def leg_a():
            return "a", timed(lambda: grp.relay(ids, counts, er, cw1, out=cw2_a, out_len=wl_a, fate=ft_a))

        def leg_b():
            def f():
                if counts is None:
                    dec.decode(ids, er, cw1, out=msg, out_len=ml)
                else:
                    dec.decode_burst(ids, counts, er, cw1, out=msg, out_len=ml)
                ml.clamp_(0, L)
                if fed >= T1:
                    if counts is None:
                        enc.encode(ids, msg, ml, out=cw2_b, out_len=wl_b)
                    else:
                        enc.encode_burst(ids, counts, msg, ml, out=cw2_b, out_len=wl_b)
                elif fed + Q > T1:  # the flows' first messages: rows T1 - fed .. Q-1 of every burst
                    lo = T1 - fed
                    sub = msg.view(NS, Q, L)[:, lo:].reshape(-1, L)
                    o, ol = enc.encode_burst(ids, np.full(NS, Q - lo, dtype=np.int32), sub, ml.view(NS, Q)[:, lo:].reshape(-1))
                    cw2_b.zero_()
                    wl_b.zero_()
                    cw2_b.view(NS, Q, -1)[:, lo:] = o.view(NS, Q - lo, -1)
                    wl_b.view(NS, Q)[:, lo:] = ol.view(NS, Q - lo)
                else:
                    cw2_b.zero_()
                    wl_b.zero_()
            return "b", timed(f)

        legs = [x for x, on in ((leg_a, "a" in LEGS), (leg_b, "b" in LEGS)) if on]
        if r % 2:
            legs.reverse()
        for leg in legs:
            name, dt = leg()
            if r >= warm:
                t[name].append(dt)
        if LEGS == "ab":
            same = same and torch.equal(cw2_a, cw2_b) and torch.equal(wl_a, wl_b)
    print(f"{NS} flows x Q = {Q} packets per flow and step ({REPEATS} repeats after {warm}):", flush=True)
    res = {}
    if "a" in LEGS:
        res["a"] = show("(a) message-wise relay group, one call ", t["a"], R)
    if "b" in LEGS:
        res["b"] = show("(b) decode_burst + clamp + encode_burst", t["b"], R)
    if LEGS == "ab":
        print(f"  outputs {'identical' if same else 'DIFFER'}", flush=True)
    return res, same


ok = True
results = {}
for NS, Q in ((10000, 1), (10000, 16), (10000, 64), (100, 1024)):
    results[(NS, Q)], same = run(NS, Q)
    ok = ok and same
if LEGS == "ab":
    for key, res in results.items():
        (a, _, _), (b, bmin, bmax) = res["a"], res["b"]
        verdict = "fused faster" if a < bmin else "FUSED SLOWER THAN THE COMPOSITION'S SLOWEST REPEAT" if a > bmax else "within the composition's spread"
        print(f"{key[0]} x {key[1]}: fused {a:.2f} against composition {b:.2f} ns per packet (min {bmin:.2f} .. max {bmax:.2f}), "
              f"{b / a:.2f}x: {verdict}")
    print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
