"""In-process A/B of the two ways to carry Q packets of every message-wise (type-1) relay flow of a node
whose flows run different pairs of codes: 10 000 flows spread evenly over the five pairs
(10,3,3)->(10,3,3), (10,5,2)->(6,2,2), (3,2,2)->(10,1,1), (4,4,4)->(10,3,3), (10,1,1)->(4,4,4) (flow s runs
pair s mod 5), 300-byte payloads, flow s's hop 1 on bin_erasure from phase 36*s, Q in {1, 16}:
  (a) one mixed group (MessageWiseRelayGroup.mixed): one relay call per round;
  (b) five one-code groups: five relay calls per round.
And what the pairs with the largest rows cost the others: the same 10 000 flows over the three pairs
without a k = 1 code ((4,4,4) on either hop: rows of 1 510 bytes, which set the five-pair group's strides,
slots and the LDS of every launch they take part in), Q in {1, 16}, in
  (a4) one mixed group against (b4) three one-code groups.
And at Q = 16 the price of the table and of the in-kernel carve-up: 10 000 flows of (10,3,3)->(10,3,3) in
  (c1) a one-code group (the argument-driven kernel) against (c2) a mixed group of that one pair.
The codeword rows are real FEC_Encoder codewords (per pair one source stream cut into Q rows per flow),
fed again every repeat: the relay does not care that a flow's rows do not continue each other.  One
process, the legs on groups in the same state fed the same rows, the legs alternating (the order swaps
every repeat), warm-up first; per leg the median (min .. max) over the repeats of the host-inclusive time
per packet: the leg's relay calls plus one synchronise.  Every repeat the legs' hop-2 codewords, sizes and
fates are compared, flow by flow over each flow's own bytes.  --mixed-only runs legs (a), (a4) and (c2)
alone.
  timeout -k 10 900 python tools/mw_relay_streams_mixed_ab.py [repeats] [--mixed-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)

torch.cuda.set_device(0)
from fec_erasure_code_unit_test_relay_amd import Codec, MessageWiseRelayGroup, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

L = 300
FIVE = [((10, 3, 3), (10, 3, 3)), ((10, 5, 2), (6, 2, 2)), ((3, 2, 2), (10, 1, 1)), ((4, 4, 4), (10, 3, 3)),
        ((10, 1, 1), (4, 4, 4))]  # PAIRS of tests/test_gpu_mw_relay_streams.py
WARM = 3
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPEATS = int(args[0]) if args else 9
MIXED_ONLY = "--mixed-only" in sys.argv
pat1 = load_pattern("bin_erasure")[:360000].astype(np.uint8)


def k_of(code):
    return code[0] - code[2] + 1


def cw_bytes(code):
    k = k_of(code)
    return -(-(L + 2) // k) * (k + code[1])


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
        self.cw = torch.zeros((n * Q, grp.cw1_bytes), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((n * Q, grp.cw2_bytes), dtype=torch.uint8, device="cuda")
        self.wl = torch.empty(n * Q, dtype=torch.int32, device="cuda")
        self.ft = torch.empty(n * Q, dtype=torch.uint8, device="cuda")

    def codewords(self, flows, cw):
        """cw [len(flows), Q, CW1]: the codewords of workload flows `flows`, all of them this leg's."""
        at = torch.from_numpy(np.searchsorted(self.members, flows)).cuda()
        self.cw.view(self.members.size, self.Q, -1)[at, :, :cw.shape[2]] = cw

    def flags(self, e1):
        self.e1 = np.ascontiguousarray(e1[self.members]).reshape(-1)

    def relay(self):
        self.grp.relay(self.ids, self.counts, self.e1, self.cw, out=self.out, out_len=self.wl, fate=self.ft)

    def rows(self, flows, CW2):
        """(hop-2 codewords[:, :, :CW2], sizes, fates) of workload flows `flows`."""
        n, Q = self.members.size, self.Q
        at = torch.from_numpy(np.searchsorted(self.members, flows)).cuda()
        return self.out.view(n, Q, -1)[at, :, :CW2], self.wl.view(n, Q)[at], self.ft.view(n, Q)[at]


def timed(legs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for leg in legs:
        leg.relay()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts, packets):
    ts = np.sort(np.array(ts)) * 1e9 / packets
    return {"ns": float(np.median(ts)), "lo": float(ts[0]), "hi": float(ts[-1])}


def show(name, t, packets):
    s = stats(t, packets)
    print(f"  {name}: relay {s['ns']:7.2f} (min {s['lo']:.2f} .. max {s['hi']:.2f}) ns per packet", flush=True)
    return s


def compare(NS, Q, pairs, code_of, legs_x, legs_y, name_x, name_y):
    """Leg x and leg y (lists of Leg, each leg serving all NS flows between its groups) on the same rows."""
    reps = WARM + REPEATS
    own = []
    for c, (code1, code2) in enumerate(pairs):  # the source's codewords, per pair
        flows = np.flatnonzero(code_of == c)
        own.append((flows, cw_bytes(code2)))
        cw, _ = Codec(L, *code1).encode(fill_payload(0, flows.size * Q, L, 0xA11 + c))
        cw = cw.view(flows.size, Q, -1)
        for leg in legs_x + legs_y:
            mine = np.isin(flows, leg.members)
            if mine.any():
                leg.codewords(flows[mine], cw[torch.from_numpy(mine).cuda()])
        del cw
    e1 = flags(pat1, 36, NS, reps * Q)
    tx, ty = [], []
    same = True
    for r in range(reps):
        for leg in legs_x + legs_y:
            leg.flags(e1[:, r * Q:(r + 1) * Q])
        order = [(legs_x, tx), (legs_y, ty)]
        if r % 2:
            order.reverse()
        for legs, t in order:
            if not legs:
                continue
            a = timed(legs)
            if r >= WARM:
                t.append(a)
        # both legs served the same rows from the same state: flow by flow the same own bytes
        for flows, CW2 in own if legs_y else []:
            for ly in legs_y:
                sel = flows[np.isin(flows, ly.members)]
                if sel.size == 0:
                    continue
                for a, b in zip(legs_x[0].rows(sel, CW2), ly.rows(sel, CW2)):
                    same = same and torch.equal(a, b)
    print(f"{NS} flows x Q = {Q} packets per flow and round ({REPEATS} repeats after {WARM}):", flush=True)
    x = show(name_x, tx, NS * Q)
    if legs_y:
        y = show(name_y, ty, NS * Q)
        gap = x["ns"] - y["ns"]
        where = "inside" if y["lo"] <= x["ns"] <= y["hi"] else "below" if gap < 0 else "ABOVE"
        print(f"  {name_x.strip()} - {name_y.strip()} = {gap:+.2f} ns per packet ({100 * gap / y['ns']:+.1f} %); the "
              f"latter's own min .. max spread {y['hi'] - y['lo']:.2f}: {where} it", flush=True)
        print(f"  outputs {'identical' if same else 'DIFFER'}", flush=True)
    return same


def mixed_against_one_code_groups(Q, pairs, tag, NS=10000):
    code_of = (np.arange(NS) % len(pairs)).astype(np.int32)
    everyone = np.arange(NS)
    a = [Leg(MessageWiseRelayGroup.mixed(L, pairs, code_of), everyone, Q)]
    b = []
    for c, pair in enumerate(pairs if not MIXED_ONLY else []):
        members = everyone[code_of == c]
        b.append(Leg(MessageWiseRelayGroup(L, *pair, members.size), members, Q))
    words = {3: "three", 5: "five"}[len(pairs)]
    return compare(NS, Q, pairs, code_of, a, b, f"(a{tag}) one mixed group    ", f"(b{tag}) {words} one-code groups")


def table_against_arguments(Q, NS=10000):
    code_of = np.zeros(NS, dtype=np.int32)
    everyone = np.arange(NS)
    c2 = [Leg(MessageWiseRelayGroup.mixed(L, FIVE[:1], code_of), everyone, Q)]
    c1 = [] if MIXED_ONLY else [Leg(MessageWiseRelayGroup(L, *FIVE[0], NS), everyone, Q)]
    return compare(NS, Q, FIVE[:1], code_of, c2, c1, "(c2) mixed, one pair ", "(c1) one-code group  ")


ok = True
for Q in (1, 16):
    ok = mixed_against_one_code_groups(Q, FIVE, "") and ok
for Q in (1, 16):
    ok = mixed_against_one_code_groups(Q, [p for p in FIVE if 1 not in (k_of(p[0]), k_of(p[1]))], "4") and ok
ok = table_against_arguments(16) and ok
if not MIXED_ONLY:
    print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
