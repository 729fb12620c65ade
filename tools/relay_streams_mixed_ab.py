"""In-process A/B of the two ways to carry Q packets of every type-2 relay flow of a node whose flows
run different codes: 10 000 flows spread evenly over the six SWDF tuples (10,3,10,3), (10,3,9,2),
(10,1,12,3), (10,10,10,10), (10,5,8,3), (6,2,10,6) (flow s runs tuple s mod 6), 300-byte payloads,
flow s's hops on bin_erasure from phase 36*s and bin_erasure2 from phase 41*s, Q in {1, 16}:
  (a) one mixed group (RelayStreamGroup.mixed): one relay call and one destination call per round;
  (b) six one-code groups: six relay calls and six destination calls per round.
And at Q = 16 the price of taking the geometry from the table: 10 000 flows of (10,3,10,3) in
  (c1) a one-code group (the argument-driven kernels) against (c2) a mixed group of that one code.
And at Q = 16 what the code with the largest rows costs the others: the same 10 000 flows over the
five tuples without (10,10,10,10) (k = 1, rows of 3 322 bytes, one chunk per CU's LDS), in
  (a5) one mixed group against (b5) five one-code groups.
The codeword rows are real FEC_Encoder codewords (per code one source stream cut into Q rows per
flow), fed again every repeat: the relay does not care that a flow's rows do not continue each
other.  One process, the legs on groups in the same state fed the same rows, the legs alternating
(the order swaps every repeat),
warm-up first; per leg the median (min .. max) over the repeats of the host-inclusive time per
packet: relay calls plus one synchronise, destination calls plus one synchronise, and their sum.
Every repeat the legs' frames, destination rows and flags are compared, flow by flow over each
flow's own bytes.  --mixed-only runs legs (a), (a5) and (c2) alone (for a kernel trace).
  timeout -k 10 900 python tools/relay_streams_mixed_ab.py [repeats] [--mixed-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)

torch.cuda.set_device(0)
from fec_erasure_code_unit_test_relay_amd import Codec, RelayStreamGroup, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

L = 300
SIX = [(10, 3, 10, 3), (10, 3, 9, 2), (10, 1, 12, 3), (10, 10, 10, 10), (10, 5, 8, 3), (6, 2, 10, 6)]
WARM = 3
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPEATS = int(args[0]) if args else 9
MIXED_ONLY = "--mixed-only" in sys.argv
pat1 = load_pattern("bin_erasure")[:360000].astype(np.uint8)
pat2 = load_pattern("bin_erasure2")[:360000].astype(np.uint8)


def flags(pat, step, NS, total):
    ph = (step * np.arange(NS, dtype=np.int64)) % pat.size
    return np.stack([pat[(ph + t) % pat.size] for t in range(total)], axis=1)  # [NS, total]


class Leg:
    """One group and the flows it serves (`members`: their numbers in the workload, in id order)."""

    def __init__(self, grp, members, Q):
        n = members.size
        self.grp, self.members, self.Q = grp, members, Q
        self.ids = np.arange(n, dtype=np.int32)
        self.counts = None if Q == 1 else np.full(n, Q, dtype=np.int32)
        self.cw = torch.zeros((n * Q, grp.cw_bytes), dtype=torch.uint8, device="cuda")
        self.fr = torch.empty((n * Q, grp.frame_bytes), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((n * Q, grp.out_bytes), dtype=torch.uint8, device="cuda")
        self.rf = torch.empty(n * Q, dtype=torch.uint8, device="cuda")
        self.df = torch.empty(n * Q, dtype=torch.uint8, device="cuda")

    def codewords(self, flows, cw):
        """cw [len(flows), Q, CW]: the codewords of workload flows `flows`, all of them this leg's."""
        at = torch.from_numpy(np.searchsorted(self.members, flows)).cuda()
        self.cw.view(self.members.size, self.Q, -1)[at, :, :cw.shape[2]] = cw

    def flags(self, e1, e2):
        self.e1 = np.ascontiguousarray(e1[self.members]).reshape(-1)
        self.e2 = np.ascontiguousarray(e2[self.members]).reshape(-1)

    def relay(self):
        self.grp.relay(self.ids, self.counts, self.e1, self.cw, frames=self.fr, flag=self.rf)

    def destination(self):
        self.grp.destination(self.ids, self.counts, self.e2, self.fr, out=self.out, flag=self.df)

    def rows(self, flows, F, OB):
        """(frames[:, :, :F], relay flags, destination rows[:, :, :OB], destination flags) of workload
        flows `flows`."""
        n, Q = self.members.size, self.Q
        at = torch.from_numpy(np.searchsorted(self.members, flows)).cuda()
        return (self.fr.view(n, Q, -1)[at, :, :F], self.rf.view(n, Q)[at],
                self.out.view(n, Q, -1)[at, :, :OB], self.df.view(n, Q)[at])


def timed(legs, what):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for leg in legs:
        getattr(leg, what)()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts, packets):
    ts = np.sort(np.array(ts)) * 1e9 / packets
    return {"ns": float(np.median(ts)), "lo": float(ts[0]), "hi": float(ts[-1])}


def show(name, t, packets):
    s = {k: stats(v, packets) for k, v in t.items()}
    print(f"  {name}: relay {s['relay']['ns']:7.2f} (min {s['relay']['lo']:.2f} .. max {s['relay']['hi']:.2f})   "
          f"destination {s['dest']['ns']:7.2f} (min {s['dest']['lo']:.2f} .. max {s['dest']['hi']:.2f})   "
          f"both {s['both']['ns']:7.2f} (min {s['both']['lo']:.2f} .. max {s['both']['hi']:.2f}) ns per packet",
          flush=True)
    return s


def compare(NS, Q, tuples, code_of, legs_x, legs_y, name_x, name_y):
    """Leg x and leg y (lists of Leg, each leg serving all NS flows between its groups) on the same rows."""
    reps = WARM + REPEATS
    ncodes = len(tuples)
    own = []
    for c, (T1, N1, T2, N2) in enumerate(tuples):  # the source's codewords, per code
        flows = np.flatnonzero(code_of == c)
        k = T1 - N1 + 1
        S = -(-(L + 2) // k)
        own.append((flows, 2 + (S + 1) * (T2 + 1), S * k))
        cw, _ = Codec(L, T1, N1, N1).encode(fill_payload(0, flows.size * Q, L, 0xA11 + c))
        cw = cw.view(flows.size, Q, -1)
        for leg in legs_x + legs_y:
            mine = np.isin(flows, leg.members)
            if mine.any():
                leg.codewords(flows[mine], cw[torch.from_numpy(mine).cuda()])
        del cw
    e1, e2 = flags(pat1, 36, NS, reps * Q), flags(pat2, 41, NS, reps * Q)
    tx = {"relay": [], "dest": [], "both": []}
    ty = {"relay": [], "dest": [], "both": []}
    same = True
    for r in range(reps):
        for leg in legs_x + legs_y:
            leg.flags(e1[:, r * Q:(r + 1) * Q], e2[:, r * Q:(r + 1) * Q])
        order = [(legs_x, tx), (legs_y, ty)]
        if r % 2:
            order.reverse()
        for legs, t in order:
            if not legs:
                continue
            a, b = timed(legs, "relay"), timed(legs, "destination")
            if r >= WARM:
                t["relay"].append(a), t["dest"].append(b), t["both"].append(a + b)
        # both legs served the same rows from the same state: flow by flow the same own bytes
        for c in range(ncodes if legs_y else 0):
            flows, F, OB = own[c]
            for ly in legs_y:
                sel = flows[np.isin(flows, ly.members)]
                if sel.size == 0:
                    continue
                for a, b in zip(legs_x[0].rows(sel, F, OB), ly.rows(sel, F, OB)):
                    same = same and torch.equal(a, b)
    print(f"{NS} flows x Q = {Q} packets per flow and round ({REPEATS} repeats after {WARM}):", flush=True)
    sx = show(name_x, tx, NS * Q)
    if legs_y:
        sy = show(name_y, ty, NS * Q)
        for side in ("relay", "dest", "both"):
            x, y = sx[side], sy[side]
            gap = x["ns"] - y["ns"]
            where = "inside" if y["lo"] <= x["ns"] <= y["hi"] else "below" if gap < 0 else "ABOVE"
            print(f"  {side}: {name_x.strip()} - {name_y.strip()} = {gap:+.2f} ns per packet; the latter's own "
                  f"min .. max spread {y['hi'] - y['lo']:.2f}: {where} it", flush=True)
        print(f"  outputs {'identical' if same else 'DIFFER'}", flush=True)
    return same


def mixed_against_one_code_groups(Q, tuples, tag, NS=10000):
    code_of = (np.arange(NS) % len(tuples)).astype(np.int32)
    everyone = np.arange(NS)
    a = [Leg(RelayStreamGroup.mixed(L, tuples, code_of), everyone, Q)]
    b = []
    for c, cfg in enumerate(tuples if not MIXED_ONLY else []):
        members = everyone[code_of == c]
        b.append(Leg(RelayStreamGroup(L, *cfg, members.size), members, Q))
    words = {5: "five", 6: "six"}[len(tuples)]
    return compare(NS, Q, tuples, code_of, a, b, f"(a{tag}) one mixed group   ", f"(b{tag}) {words} one-code groups")


def table_against_arguments(Q, NS=10000):
    code_of = np.zeros(NS, dtype=np.int32)
    everyone = np.arange(NS)
    c2 = [Leg(RelayStreamGroup.mixed(L, SIX[:1], code_of), everyone, Q)]
    c1 = [] if MIXED_ONLY else [Leg(RelayStreamGroup(L, *SIX[0], NS), everyone, Q)]
    return compare(NS, Q, SIX[:1], code_of, c2, c1, "(c2) mixed, one code ", "(c1) one-code group  ")


ok = True
for Q in (1, 16):
    ok = mixed_against_one_code_groups(Q, SIX, "") and ok
ok = mixed_against_one_code_groups(16, [t for t in SIX if t != (10, 10, 10, 10)], "5") and ok
ok = table_against_arguments(16) and ok
if not MIXED_ONLY:
    print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
