"""In-process A/B of the two ways to code Q packets of every stream of a node whose streams run
different codes: 10 000 streams spread evenly over the six T = 10 tuples (10,3,3), (10,5,2), (10,1,1),
(10,0,0), (10,2,1), (10,4,4) (stream s runs tuple s mod 6), 300-byte payloads, stream s on
bin_erasure from phase 36*s, Q in {1, 16}:
  (a) one mixed group (StreamGroup.mixed): one encode call and one decode call per round;
  (b) six one-code groups: six encode calls and six decode calls per round.
And at Q = 16 the price of taking the geometry from the table: 10 000 streams of (10,3,3) in
  (c1) a one-code group (the burst kernels) against (c2) a mixed group of that one code.
One process, the legs on groups in the same state fed the same packets, the legs alternating (the
order swaps every repeat), warm-up first; per leg the median (min .. max) over the repeats of the
host-inclusive time per round and per packet.  Every repeat the legs' rows and lengths are compared.
  python tools/streams_mixed_ab.py [repeats]"""
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

L = 300
SIX = [(10, 3, 3), (10, 5, 2), (10, 1, 1), (10, 0, 0), (10, 2, 1), (10, 4, 4)]
WARM = 3
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
base = load_pattern("bin_erasure")[:360000].astype(np.uint8)


class Leg:
    """One group and the streams it serves (`members`: their numbers in the workload, in id order)."""

    def __init__(self, grp, members, Q):
        n = members.size
        self.grp, self.members, self.Q = grp, members, Q
        self.ids = np.arange(n, dtype=np.int32)
        self.counts = np.full(n, Q, dtype=np.int32)
        self.cw = torch.empty((n * Q, grp.CW), dtype=torch.uint8, device="cuda")
        self.wl = torch.empty(n * Q, dtype=torch.int32, device="cuda")
        self.out = torch.empty((n * Q, L), dtype=torch.uint8, device="cuda")
        self.ol = torch.empty(n * Q, dtype=torch.int32, device="cuda")

    def data(self, pay, er):
        """pay [NS, Q, L] on the device, er [NS, Q] host flags of this repeat."""
        self.pay = pay[torch.from_numpy(self.members).cuda()].reshape(-1, L).contiguous()
        self.er = np.ascontiguousarray(er[self.members]).reshape(-1)

    def run(self):
        g = self.grp
        if self.Q == 1:
            g.encode(self.ids, self.pay, out=self.cw, out_len=self.wl)
            g.decode(self.ids, self.er, self.cw, out=self.out, out_len=self.ol)
        else:
            g.encode_burst(self.ids, self.counts, self.pay, out=self.cw, out_len=self.wl)
            g.decode_burst(self.ids, self.counts, self.er, self.cw, out=self.out, out_len=self.ol)

    def rows(self, s_sel, CW):
        """(cw[:, :, :CW], sizes, payload rows, lengths) of the group's streams s_sel, [len, Q, ...]."""
        n, Q = self.members.size, self.Q
        return (self.cw.view(n, Q, -1)[s_sel, :, :CW], self.wl.view(n, Q)[s_sel],
                self.out.view(n, Q, L)[s_sel], self.ol.view(n, Q)[s_sel])


def stats(ts, packets):
    ts = np.sort(np.array(ts))
    return {"us": float(np.median(ts)) * 1e6, "ns": float(np.median(ts)) * 1e9 / packets,
            "lo": float(ts[0]) * 1e9 / packets, "hi": float(ts[-1]) * 1e9 / packets}


def show(name, s):
    print(f"  {name}: {s['us']:9.1f} us per round   {s['ns']:7.3f} ns per packet "
          f"(min {s['lo']:.3f} .. max {s['hi']:.3f})", flush=True)


def compare(NS, Q, tuples, code_of, legs_x, legs_y, name_x, name_y):
    """Leg x and leg y (lists of Leg, each leg serving all NS streams between its groups) on the same packets."""
    reps = WARM + REPEATS
    pay = fill_payload(0, NS * Q, L, 0xA11).view(NS, Q, L)
    ph = (36 * np.arange(NS, dtype=np.int64)) % base.size
    er = np.stack([base[(ph + t) % base.size] for t in range(reps * Q)], axis=1)  # [NS, reps * Q]
    tx, ty, same = [], [], True
    for r in range(reps):
        for leg in legs_x + legs_y:
            leg.data(pay, er[:, r * Q:(r + 1) * Q])
        order = [(legs_x, tx), (legs_y, ty)]
        if r % 2:
            order.reverse()
        for legs, ts in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for leg in legs:
                leg.run()
            torch.cuda.synchronize()
            if r >= WARM:
                ts.append(time.perf_counter() - t0)
        # both legs coded the same packets from the same state: stream by stream the same rows
        for ly in legs_y:
            for lx in legs_x:
                sel_x = np.flatnonzero(np.isin(lx.members, ly.members))
                if sel_x.size == 0:
                    continue
                sel_y = np.searchsorted(ly.members, lx.members[sel_x])
                for c in np.unique(code_of[lx.members[sel_x]]):
                    T, B, N = tuples[c]
                    CW = -(-(L + 2) // (T - N + 1)) * (T - N + 1 + B)
                    m = code_of[lx.members[sel_x]] == c
                    for a, b in zip(lx.rows(torch.from_numpy(sel_x[m]).cuda(), CW),
                                    ly.rows(torch.from_numpy(sel_y[m]).cuda(), CW)):
                        same = same and torch.equal(a, b)
    print(f"{NS} streams x Q = {Q} packets per stream and round ({REPEATS} repeats after {WARM}):", flush=True)
    sx, sy = stats(tx, NS * Q), stats(ty, NS * Q)
    show(name_x, sx)
    show(name_y, sy)
    gap = sx["ns"] - sy["ns"]
    print(f"  {name_x.strip()} - {name_y.strip()} = {gap:+.3f} ns per packet; the latter's own min .. max spread "
          f"{sy['hi'] - sy['lo']:.3f}: {'inside' if sy['lo'] <= sx['ns'] <= sy['hi'] else 'below' if gap < 0 else 'ABOVE'}"
          f" it; outputs {'identical' if same else 'DIFFER'}", flush=True)
    return same


def mixed_against_six(Q, NS=10000):
    code_of = (np.arange(NS) % 6).astype(np.int32)
    everyone = np.arange(NS)
    a = [Leg(StreamGroup.mixed(L, SIX, code_of), everyone, Q)]
    b = []
    for c, (T, B, N) in enumerate(SIX):
        members = everyone[code_of == c]
        b.append(Leg(StreamGroup(L, T, B, N, members.size), members, Q))
    return compare(NS, Q, SIX, code_of, a, b, "(a) one mixed group   ", "(b) six one-code groups")


def table_against_arguments(Q, NS=10000):
    code_of = np.zeros(NS, dtype=np.int32)
    everyone = np.arange(NS)
    c2 = [Leg(StreamGroup.mixed(L, SIX[:1], code_of), everyone, Q)]
    c1 = [Leg(StreamGroup(L, 10, 3, 3, NS), everyone, Q)]
    return compare(NS, Q, SIX[:1], code_of, c2, c1, "(c2) mixed, one code ", "(c1) one-code group  ")


ok = True
for Q in (1, 16):
    ok = mixed_against_six(Q) and ok
ok = table_against_arguments(16) and ok
print("outputs identical on every workload" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
