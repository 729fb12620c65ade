"""In-process A/B of the two ways to carry many type-2 relay flows, Q packets of every flow per step:
  (a) a relay stream group (RelayStreamGroup): one relay call and one destination call for all the
      flows, at 10 000 flows, Q in {1, 16, 64} (Q = 1: one-packet calls, counts = None);
  (b) without the group: per flow one SymbolWiseRelay.relay over H1 + Q rows, the flow's last
      H1 = n1 + n2 - 2 codewords and flags fed again in front (and one .destination over H2 + Q frames,
      H2 = n2 - 1), the history rows of the result thrown away, at the first 1 000 of those flows.
(10,3,10,3), 300-byte payloads; flow s's hops on bin_erasure from phase 36*s and bin_erasure2 from
phase 41*s.  The codeword rows are real FEC_Encoder codewords of Q packets per flow, fed again every
repeat (the relay does not care that the repeats do not form one source stream).  One process, both
legs fed the same rows from the same state, the legs alternating (the order swaps every repeat),
warm-up first; per leg and side the median (min .. max) over the repeats of the host-inclusive time
per packet, calls plus one synchronise.  After every repeat leg (b)'s rows must equal leg (a)'s rows
of the same flows.  --group-only runs leg (a) alone (for a kernel trace).
  timeout -k 10 900 python tools/relay_streams_ab.py [repeats] [--group-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)

torch.cuda.set_device(0)
from fec_erasure_code_unit_test_relay_amd import RelayStreamGroup, StreamGroup, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.relay import SymbolWiseRelay  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

L, CFG = 300, (10, 3, 10, 3)
NS, NB = 10000, 1000
WARM = 3
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPEATS = int(args[0]) if args else 9
GROUP_ONLY = "--group-only" in sys.argv
pat1 = load_pattern("bin_erasure")[:360000].astype(np.uint8)
pat2 = load_pattern("bin_erasure2")[:360000].astype(np.uint8)


def flags(pat, step, total):
    ph = (step * np.arange(NS, dtype=np.int64)) % pat.size
    return np.stack([pat[(ph + t) % pat.size] for t in range(total)], axis=1)  # [NS, total]


def show(name, ts, packets):
    ts = np.sort(np.array(ts)) * 1e9 / packets
    print(f"  {name}: {float(np.median(ts)):9.2f} ns per packet (min {ts[0]:.2f} .. max {ts[-1]:.2f})", flush=True)
    return float(np.median(ts))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(Q):
    reps = WARM + REPEATS
    ids = np.arange(NS, dtype=np.int32)
    counts = None if Q == 1 else np.full(NS, Q, dtype=np.int32)
    src = StreamGroup(L, CFG[0], CFG[1], CFG[1], NS)
    cw, _ = src.encode_burst(ids, np.full(NS, Q, dtype=np.int32), fill_payload(0, NS * Q, L, 0xA11))
    del src
    e1, e2 = flags(pat1, 36, reps * Q), flags(pat2, 41, reps * Q)
    grp = RelayStreamGroup(L, *CFG, NS)
    F, SK, CW = grp.frame_bytes, grp.S * grp.k, grp.cw_bytes
    fr = torch.empty((NS * Q, F), dtype=torch.uint8, device="cuda")
    out = torch.empty((NS * Q, SK), dtype=torch.uint8, device="cuda")
    rf = torch.empty(NS * Q, dtype=torch.uint8, device="cuda")
    df = torch.empty(NS * Q, dtype=torch.uint8, device="cuda")
    if not GROUP_ONLY:
        sw = SymbolWiseRelay(L, *CFG)
        H1, H2 = grp.n1 + grp.n2 - 2, grp.n2 - 1
        # the flows' last H rows and flags (zero rows, not erased, before a flow's first packet)
        h_cw = torch.zeros((NB, H1, CW), dtype=torch.uint8, device="cuda")
        h_fr = torch.zeros((NB, H2, F), dtype=torch.uint8, device="cuda")
        h_e1, h_e2 = np.zeros((NB, H1), dtype=np.uint8), np.zeros((NB, H2), dtype=np.uint8)
        fr_b = torch.empty((NB, H1 + Q, F), dtype=torch.uint8, device="cuda")
        rf_b = torch.empty((NB, H1 + Q), dtype=torch.uint8, device="cuda")
        out_b = torch.empty((NB, H2 + Q, SK), dtype=torch.uint8, device="cuda")
        df_b = torch.empty((NB, H2 + Q), dtype=torch.uint8, device="cuda")
    t = {"a_relay": [], "a_dest": [], "b_relay": [], "b_dest": []}
    same = True
    for r in range(reps):
        b1, b2 = e1[:, r * Q:(r + 1) * Q], e2[:, r * Q:(r + 1) * Q]
        f1, f2 = np.ascontiguousarray(b1).reshape(-1), np.ascontiguousarray(b2).reshape(-1)

        def leg_a():
            ta = timed(lambda: grp.relay(ids, counts, f1, cw, frames=fr, flag=rf))
            tb = timed(lambda: grp.destination(ids, counts, f2, fr, out=out, flag=df))
            return ("a_relay", ta), ("a_dest", tb)

        def leg_b():
            in_cw = torch.cat([h_cw, cw.view(NS, Q, CW)[:NB]], dim=1)
            in_e1 = torch.from_numpy(np.concatenate([h_e1, b1[:NB]], axis=1)).cuda()
            in_e2 = torch.from_numpy(np.concatenate([h_e2, b2[:NB]], axis=1)).cuda()

            def relay_b():
                for s in range(NB):
                    sw.relay(in_cw[s], in_e1[s], frames=fr_b[s], flag=rf_b[s])

            ta = timed(relay_b)
            in_fr = torch.cat([h_fr, fr_b[:, H1:]], dim=1)

            def dest_b():
                for s in range(NB):
                    sw.destination(in_fr[s], in_e2[s], out=out_b[s], flag=df_b[s])

            tb = timed(dest_b)
            h_cw.copy_(in_cw[:, Q:])
            h_fr.copy_(in_fr[:, Q:])
            h_e1[:], h_e2[:] = in_e1[:, Q:].cpu().numpy(), in_e2[:, Q:].cpu().numpy()
            return ("b_relay", ta), ("b_dest", tb)

        legs = [leg_a] if GROUP_ONLY else [leg_a, leg_b]
        if r % 2:
            legs.reverse()
        for leg in legs:
            for name, dt in leg():
                if r >= WARM:
                    t[name].append(dt)
        if not GROUP_ONLY:  # leg (b)'s rows behind the history = leg (a)'s rows of the same flows
            same = same and torch.equal(fr_b[:, H1:], fr.view(NS, Q, F)[:NB]) \
                and torch.equal(rf_b[:, H1:], rf.view(NS, Q)[:NB]) \
                and torch.equal(out_b[:, H2:], out.view(NS, Q, SK)[:NB]) \
                and torch.equal(df_b[:, H2:], df.view(NS, Q)[:NB])
    print(f"Q = {Q} packets per flow and step ({REPEATS} repeats after {WARM}):", flush=True)
    res = {"a_relay": show(f"(a) group, {NS} flows, relay      ", t["a_relay"], NS * Q),
           "a_dest": show(f"(a) group, {NS} flows, destination", t["a_dest"], NS * Q)}
    if not GROUP_ONLY:
        res["b_relay"] = show(f"(b) per flow, {NB} flows, relay      ", t["b_relay"], NB * Q)
        res["b_dest"] = show(f"(b) per flow, {NB} flows, destination", t["b_dest"], NB * Q)
        print(f"  outputs {'identical' if same else 'DIFFER'}", flush=True)
    return res, same


results, ok = {}, True
for Q in (1, 16, 64):
    results[Q], same = run(Q)
    ok = ok and same
for side in ("relay", "dest"):
    a1, a16 = results[1]["a_" + side], results[16]["a_" + side]
    print(f"{side}: bursts of 16 against one-packet group calls: {a16:.2f} against {a1:.2f} ns per packet: "
          f"{'bursts faster' if a16 < a1 else 'BURSTS NOT FASTER'}")
    if not GROUP_ONLY:
        b16 = results[16]["b_" + side]
        print(f"{side}: the group at Q = 16 against one batch per flow: {a16:.2f} against {b16:.2f} ns per packet "
              f"({b16 / a16:.1f}x): {'group faster' if a16 < b16 else 'GROUP NOT FASTER'}")
if not GROUP_ONLY:
    print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
