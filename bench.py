"""bench.py -- device-resident GF(2^8) streaming-erasure encode+decode throughput on MI355X.

Metric (BASELINE.json): GiB/s of device-resident erasure encode+decode, 300-byte packets, T=10,
and its fraction of the HBM roofline.  One step = one pass of the hot path over one batch: encode
P+T packets of a fresh stream ((T,B,N) = (10,3,3), 300-byte synthetic payloads), erase with the
reference's recorded pattern bin/erasure.bin (replayed, ERASURE_TYPE=5 semantics), decode with a
fresh decoder -> the reference's output for P packets.  Inputs are resident in HBM before timing.

Multi-GPU (torchrun, one process per GPU): weak scaling, one independent stream per GPU (seed and
pattern phase per rank); no collective in the data path -- RCCL only for the barrier, the
max-over-ranks time and the final counter reduction.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--packets P] [--tbn 10,3,3]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line (`value`,
`ms_per_step`).  --full adds everything else to the line: the check of the timed work against its
payloads, per-kernel durations and the roofline (with a rocprofv3 child run), the host-inclusive
rates, BASELINE configs 3 and 4, the relay and multi-stream legs and the CPU baseline.
--dump-outputs DIR writes what the last timed step returned (dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np  # noqa: F401

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from fec_erasure_code_unit_test_relay_amd.streams import (max_over_ranks, reduce_counters,  # noqa: E402
                                                            stream_pattern, stream_seed)

L = 300
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md


def kernel_sources_digest():
    """SHA-256 over every source of libfec_amd.so (csrc/*.hip, *.h, *.cpp and include/*.h): a PMC
    traffic figure or a rocprof duration is only valid for the library it was measured on -- the
    host files launch kernels too (fec_vr.cpp config 4's, fec_host.cpp builds the rule tables the
    planner kernels read)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "fec_erasure_code_unit_test_relay_amd", "csrc")
    paths = [p for ext in ("*.hip", "*.h", "*.cpp") for p in glob.glob(os.path.join(csrc, ext))]
    paths += glob.glob(os.path.join(ROOT, "include", "*.h"))
    for path in sorted(paths, key=os.path.basename):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def pmc_traffic(kernel_symbol):
    """HBM bytes per launch of `kernel_symbol` from the newest committed rocprofv3 FETCH_SIZE /
    WRITE_SIZE passes (profiles/*/*_traffic.json, made by tools/pmc_traffic.{sh,py} over the same
    step at the same size).  Returns (bytes, source, fresh): fresh is False when the pass was made
    on other kernel sources than the ones built here (then the figure is not reported)."""
    import glob
    best = None
    digest = kernel_sources_digest()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "*_traffic.json"))):
        with open(path) as f:
            entry = json.load(f).get(kernel_symbol)
        if entry:
            cand = (entry["traffic_bytes"], os.path.relpath(path, ROOT), entry.get("sources_sha256") == digest)
            if best is None or cand[2] or not best[2]:  # a pass on these sources wins over any other
                best = cand
    return best


def rocprof_child(argv, symbols, keep_dir=None, timeout=300):
    """This bench's own step, re-run as a child process under `rocprofv3 --kernel-trace --stats`
    (--rocprof-child: warm-up and timed steps only, no other legs): the average duration of each
    kernel in `symbols` as the profiler sees it on this box, in this invocation -- the roofline's
    kernel time.  Returns ({symbol: {"avg_us", "calls", "min_us", "max_us"}}, info) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    out = os.path.abspath(keep_dir) if keep_dir else tempfile.mkdtemp(prefix="bench_rocprof_", dir="/tmp")
    os.makedirs(out, exist_ok=True)
    env = dict(os.environ, TMPDIR="/tmp")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "bench", "--",
           sys.executable, os.path.abspath(__file__)] + argv + ["--rocprof-child"]
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None, f"rocprofv3 child timed out after {timeout} s"
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if r.returncode != 0 or not stats:
        return None, f"rocprofv3 child exit {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
    res = {}
    for row in csv.DictReader(open(stats[-1])):
        name = row["Name"].split("(")[0].replace("void ", "").replace("fec::", "").strip()
        st = {"avg_us": float(row["AverageNs"]) / 1e3, "calls": int(row["Calls"]),
              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        res.setdefault("__all__", {})[name] = st  # every kernel (the relay legs' lookups)
        for sym in symbols:
            if sym and name == sym:
                res[sym] = st
    if not keep_dir:
        shutil.rmtree(out, ignore_errors=True)
    return res, os.path.relpath(stats[-1], ROOT) if keep_dir else "temporary"


def cpu_baseline(T, B, N, packets, rank_pattern, threads=None):
    """The oracle's reference-structured encoder+decoder on a bounded sample: one stream per
    thread (the reference is single-threaded; BASELINE.md §2 plans 1 core and one stream per
    core), each thread on its own phase of the replayed pattern.  ctypes drops the GIL during the
    C call, so the threads run on separate cores.  Reports the multi-core aggregate, with the
    1-core run beside it."""
    import threading
    import oracle
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    nth = threads or max(1, min(16, avail))  # the GPU box grants 16 cores to a job

    def one(i, res):
        off = (i * 37_001) % max(1, rank_pattern.size - packets - T)
        pat = rank_pattern[off: off + packets + T]
        r = oracle.run_stream(L, T, B, N, packets, pat, seed=0x5EED + i, want_data=False)
        res[i] = (int(pat[:packets].sum()), r["lost"])

    res1 = {}
    t0 = time.perf_counter()
    one(0, res1)
    dt1 = time.perf_counter() - t0
    resn = {}
    t0 = time.perf_counter()
    ths = [threading.Thread(target=one, args=(i, resn)) for i in range(nth)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    dtn = time.perf_counter() - t0
    return {"value": nth * packets * L / dtn / 2**30, "unit": "GiB/s", "cores": nth, "kind": "port",
            "sample": f"oracle (reference-structured C restatement, oracle/fec_oracle.c) encode+decode, "
                      f"(T,B,N)=({T},{B},{N}), {nth} independent streams (one per thread) of {packets} "
                      f"packets each on phases of the replayed bin/erasure.bin stream, {dtn:.1f} s wall",
            "seconds": dtn,
            "single_core": {"value": packets * L / dt1 / 2**30, "cores": 1, "seconds": dt1,
                            "erased": res1[0][0], "lost": res1[0][1]}}


def host_inclusive(codec, payload, pat, er, cw, wl, out, ol, P, Pf, world, barrier, max_time, reduce):
    """End-to-end rate from/to pinned host memory on every rank (north_star: the path starts and
    ends in UDP socket buffers): H2D payload, encode, D2H wire codewords, H2D codewords + erasures,
    decode, D2H payloads + lengths.  Each rank drives its own GPU's PCIe link; the job's time is the
    slowest rank's between two barriers, and `value` is the payload of all ranks over that time."""
    import torch
    from fec_erasure_code_unit_test_relay_amd import DecodeStream
    h_payload = payload.cpu().pin_memory()
    h_cw = torch.empty_like(cw, device="cpu").pin_memory()
    h_wl = torch.empty_like(wl, device="cpu").pin_memory()
    h_out = torch.empty_like(out, device="cpu").pin_memory()
    h_ol = torch.empty_like(ol, device="cpu").pin_memory()
    h_er = torch.from_numpy(pat).pin_memory()
    d_in = torch.empty_like(payload)
    d_cw2 = torch.empty_like(cw)
    d_er2 = torch.empty_like(er)

    def host_step():
        d_in.copy_(h_payload, non_blocking=True)
        codec.encode(d_in, out=cw, out_len=wl)
        h_cw.copy_(cw, non_blocking=True)
        h_wl.copy_(wl, non_blocking=True)
        d_cw2.copy_(h_cw, non_blocking=True)
        d_er2.copy_(h_er, non_blocking=True)
        codec.decode(d_cw2, d_er2, out=out, out_len=ol)
        h_out.copy_(out, non_blocking=True)
        h_ol.copy_(ol, non_blocking=True)

    # The same work in NC chunks on two streams, one per PCIe direction, software-pipelined
    # (chunk i+1 goes up and is encoded while chunk i's codewords come down): the encoder sees
    # the chunk in front as history, the decoder is the continuing one
    # (fec_decode_stream_push), so the outputs are the one-shot decode's.  Measured on the box
    # (tools/pcie_duplex.py): one large H2D and one large D2H on two streams do not overlap
    # (57 GB/s together, as either alone); interleaved 64 MB chunks reach 83 GB/s.  4 chunks
    # beat 8, 16 and 32 here (tools/host_pipe_exp.py: 21.4 / 26.6 / 39.1 / 38.5 ms).
    NC = 4
    cuts = [Pf * i // NC for i in range(NC + 1)]
    s_up, s_dn = torch.cuda.Stream(), torch.cuda.Stream()

    def host_step_pipelined():
        ds = DecodeStream(codec)
        cur = torch.cuda.current_stream()
        s_up.wait_stream(cur)
        s_dn.wait_stream(cur)
        ev_d = [None] * NC
        nout = [0]

        def send(i):
            a, b = cuts[i], cuts[i + 1]
            with torch.cuda.stream(s_up):
                d_in[a:b].copy_(h_payload[a:b], non_blocking=True)
                h = min(a, codec.n - 1)
                codec.encode(d_in[a - h:b], history=h, out=cw[a:b], out_len=wl[a:b])
                ev = torch.cuda.Event()
                ev.record()
            with torch.cuda.stream(s_dn):
                s_dn.wait_event(ev)
                h_cw[a:b].copy_(cw[a:b], non_blocking=True)
                h_wl[a:b].copy_(wl[a:b], non_blocking=True)
                ev_d[i] = torch.cuda.Event()
                ev_d[i].record()

        def receive(i):
            a, b = cuts[i], cuts[i + 1]
            n0 = nout[0]
            with torch.cuda.stream(s_up):
                s_up.wait_event(ev_d[i])
                d_cw2[a:b].copy_(h_cw[a:b], non_blocking=True)
                d_er2[a:b].copy_(h_er[a:b], non_blocking=True)
                o, _ = ds.push(d_cw2[:b], d_er2[:b], pat[:b], history=a, out=out[n0:], out_len=ol[n0:])
                ev = torch.cuda.Event()
                ev.record()
            m = o.shape[0]
            with torch.cuda.stream(s_dn):
                s_dn.wait_event(ev)
                h_out[n0:n0 + m].copy_(out[n0:n0 + m], non_blocking=True)
                h_ol[n0:n0 + m].copy_(ol[n0:n0 + m], non_blocking=True)
            nout[0] += m

        send(0)
        for i in range(NC):
            if i + 1 < NC:
                send(i + 1)
            receive(i)
        cur.wait_stream(s_up)
        cur.wait_stream(s_dn)
        return nout[0]

    # Zero-copy: the encoder reads the pinned payload rows and writes the pinned codeword rows,
    # the decoder reads those rows and the pinned erasure flags and writes the pinned payload rows
    # -- no staging copies; every kernel has both PCIe directions in flight (encode: 300 B up
    # and 418 B down per packet, decode the reverse), which the SDMA copies above cannot do
    # (tools/pcie_duplex.py).  Encode and decode of different chunks on two streams measured
    # slower (tools/host_zero_copy_exp.py: 18.1 ms one-shot vs 18.8 / 19.6 / 21.2 ms for 2 / 4 /
    # 8 chunks): each kernel alone already keeps ~80 GB/s of the ~86 GB/s duplex ceiling busy.
    import ctypes
    from fec_erasure_code_unit_test_relay_amd._lib import lib
    vp = ctypes.c_void_p
    h_er_t = torch.from_numpy(pat).pin_memory()
    ws = codec.workspace(Pf)

    def zero_copy_step():
        st = vp(torch.cuda.current_stream().cuda_stream)
        r = lib().fec_encode_batch(codec._h, vp(h_payload.data_ptr()), None, 0, Pf, vp(h_cw.data_ptr()),
                                   vp(h_wl.data_ptr()), st)
        r = r or lib().fec_decode_batch(codec._h, vp(h_cw.data_ptr()), vp(h_er_t.data_ptr()), Pf,
                                        vp(h_out.data_ptr()), vp(h_ol.data_ptr()), vp(ws.data_ptr()),
                                        ws.numel(), st)
        if r:
            raise RuntimeError(f"zero-copy encode/decode failed: {r}")
        return P

    def timed_all(fn, reps):
        fn()
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        barrier()
        return max_time((time.perf_counter() - t0) / reps), r

    hs = 3
    he, _ = timed_all(host_step, hs)
    ref_out, ref_ol, ref_cw = h_out.clone(), h_ol.clone(), h_cw.clone()
    h_out.zero_()
    hp, nout = timed_all(host_step_pipelined, hs)
    pipe_ok = nout == P and bool(torch.equal(h_out, ref_out)) and bool(torch.equal(h_ol, ref_ol))
    h_out.zero_()
    h_cw.zero_()
    hz, _ = timed_all(zero_copy_step, hs)
    zc_ok = bool(torch.equal(h_out, ref_out)) and bool(torch.equal(h_ol, ref_ol)) and bool(
        torch.equal(h_cw, ref_cw))
    # the serialised run's output against the source payloads (lost rows are zero-length)
    ok_rows = ref_ol != 0
    ser_ok = bool(torch.equal(ref_out[ok_rows], h_payload[:P][ok_rows]))
    (verified_ranks,) = reduce([int(pipe_ok and ser_ok and zc_ok)])
    gib = world * P * L / 2**30
    # Both transports are complete runs of the workload with checked outputs; which one wins
    # depends on the box's PCIe path (zero-copy 15.3 - 15.5 GiB/s on every box so far, the SDMA
    # pipeline 12.8 - 15.9), so `value` is the faster one and `method` names it.
    best = min(hz, hp)
    return {"value": round(gib / best, 3), "unit": "GiB/s",
            "ms_per_step": round(best * 1e3, 3), "n_gpus": world,
            "method": "zero_copy" if hz <= hp else "sdma_pipelined",
            "note": f"pinned host buffers (the socket side); value = payload of all {world} rank(s) / "
                    f"slowest rank's time, the faster of the two transports below; outputs checked "
                    f"equal across all three runs and against the source payloads",
            "verified": verified_ranks == world,
            "zero_copy": {"value": round(gib / hz, 3), "ms_per_step": round(hz * 1e3, 3),
                          "note": "per rank: encode reading the host payload rows and writing the host "
                                  "codeword rows, decode reading those and the host erasure flags and "
                                  "writing the host payload rows (both PCIe directions in every kernel)"},
            "sdma_pipelined": {"value": round(gib / hp, 3), "ms_per_step": round(hp * 1e3, 3),
                               "note": f"H2D payload, encode, D2H codewords, H2D codewords + erasures, "
                                       f"continuing decode, D2H payloads + lengths in {NC} chunks on 2 "
                                       f"streams"},
            "sdma_serialised_one_stream": {"value": round(gib / he, 3),
                                           "ms_per_step": round(he * 1e3, 3)}}


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


DUMP_ROWS = 8192      # sampled rows of the codeword and payload arrays (whole rows, every byte)
DUMP_PACKETS = 1 << 20  # per-packet arrays are written whole up to this many packets


def dump_outputs(dirname, cw, wl, out, ol, suffix=""):
    """--dump-outputs: what the last timed step handed its caller -- the encoder's codewords and
    wire sizes, the decoder's payload rows and lengths -- as DIR/<name>.npy, under 64 MB in all at
    the default size: the two length arrays whole (float32), a position-weighted byte sum of every
    codeword and payload row (float64, exact: below 2^31), and DUMP_ROWS whole rows of each array at
    fixed, seeded row numbers (float32).  Arrays longer than their limit are sampled the same way.
    The inputs depend on the arguments alone, so two builds can be compared file by file."""
    import torch
    os.makedirs(dirname, exist_ok=True)

    def sample(x, limit, seed):
        if x.shape[0] <= limit:
            return x
        idx = np.sort(np.random.default_rng(seed).choice(x.shape[0], limit, replace=False))
        return x[torch.from_numpy(idx).to(x.device)]

    def row_sums(x, chunk=65536):
        w = torch.arange(1, x.shape[1] + 1, device=x.device, dtype=torch.int32)
        return torch.cat([(x[a:a + chunk].to(torch.int32) * w).sum(1, dtype=torch.int64)
                          for a in range(0, x.shape[0], chunk)])

    arrays = {"wire_sizes": (sample(wl, DUMP_PACKETS, 1), np.float32),
              "payload_lengths": (sample(ol, DUMP_PACKETS, 2), np.float32),
              "codeword_row_sums": (sample(row_sums(cw), DUMP_PACKETS, 1), np.float64),
              "payload_row_sums": (sample(row_sums(out), DUMP_PACKETS, 2), np.float64),
              "codewords_sample": (sample(cw, DUMP_ROWS, 3), np.float32),
              "payloads_sample": (sample(out, DUMP_ROWS, 4), np.float32)}
    for name, (t, dt) in arrays.items():
        np.save(os.path.join(dirname, name + suffix + ".npy"), t.cpu().numpy().astype(dt))


def quiet_cpu_group(sample_s=0.2):
    """The aligned group of 8 allowed CPUs (with their SMT siblings) that was least busy over a
    short /proc/stat sample, or None.  The GPU box's host is shared: config 4's host plan places its
    threads on the calling thread's group of 8 CPUs (fec_vr.cpp, vr_pin_near), and on a busy group
    its control loop ran 1.07 vs 1.67 ms (profiles/r04/vr/r04zp_plan_spin_ab.txt)."""
    def busy():
        out = {}
        with open("/proc/stat") as f:
            for line in f:
                if line.startswith("cpu") and line[3].isdigit():
                    v = [int(x) for x in line.split()[1:]]
                    out[int(line.split()[0][3:])] = (sum(v) - v[3] - (v[4] if len(v) > 4 else 0), sum(v))
        return out
    try:
        allowed = os.sched_getaffinity(0)
        a = busy()
        time.sleep(sample_s)
        b = busy()
    except (OSError, AttributeError, ValueError, IndexError):
        return None
    load = {c: (b[c][0] - a[c][0]) / max(1, b[c][1] - a[c][1]) for c in b if c in a}
    ncpu = max(load) + 1 if load else 0
    best = None
    for base in range(0, ncpu, 8):
        group = [c for c in range(base, base + 8) if c in allowed]
        if len(group) < 8:
            continue
        # SMT siblings share the cores: count their load too (cpu c and c +- ncpu/2 on this host)
        sib = [(c + ncpu // 2) % ncpu for c in group] if ncpu >= 16 else []
        score = sum(load.get(c, 1.0) for c in group + sib)
        if best is None or score < best[0]:
            best = (score, group)
    return best[1] if best else None


def extra_configs(steps=5, kprof=None):
    """BASELINE configs 3 and 4 (parity cases, reported beside the headline, never as `value`):
    device-resident decode at (10,5,2) on bin/erasure.bin (P = 360000, the reference's pattern
    replayed from packet 0) and the adaptive variable-rate loop's schedule (encode + decode of
    every packet, mixed (T,B,N) instances) on the same pattern.  Each is verified after timing."""
    import torch
    from fec_erasure_code_unit_test_relay_amd import Codec, fill_payload
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    from fec_erasure_code_unit_test_relay_amd.vr import VrPlan
    pat = load_pattern("bin_erasure")
    P = 360000
    res = {}
    # config 3: decode (10,5,2), expected 565 lost
    c = Codec(L, 10, 5, 2)
    payload = fill_payload(0, P + 10, L, 0x5EED)
    cw, _ = c.encode(payload)
    er = torch.from_numpy(pat[:P + 10].copy()).cuda()
    out = torch.empty((P, L), dtype=torch.uint8, device="cuda")
    ol = torch.empty(P, dtype=torch.int32, device="cuda")
    c.workspace(P + 10)
    dt = timed(lambda: c.decode(cw, er, out=out, out_len=ol), steps)
    ok = ol != 0
    res["config3_decode_10_5_2"] = {
        "GiB_s": round(P * L / dt / 2**30, 2), "ms": round(dt * 1e3, 4), "packets": P,
        "lost": int((~ok).sum()), "expected_lost": 565,
        "verified": bool(torch.equal(out[ok], payload[:P][ok])) and int((~ok).sum()) == 565}
    # config 4: adaptive variable-rate loop.  One step = the symbolic host plan of the whole
    # P2P loop (fec_vr_plan_create: sender, estimators, switches, decoder instances) + its table
    # uploads + the batched device encode and decode of every packet; the plan is part of the
    # timed work.
    v = VrPlan(pat, P)
    pl = fill_payload(0, v.sent, L, 0x5EED)
    frames = v.alloc_frames(zero=False)
    out4 = torch.empty((P, L), dtype=torch.uint8, device="cuda")
    ol4 = torch.empty(P, dtype=torch.int32, device="cuda")

    # One plan object, planned again from scratch every step (fec_vr_plan_rerun reuses its host
    # buffers, device tables and threads).  The rerun returns after the serial control loop; the
    # symbolic decoder instances then run on host threads while the GPU encodes, and the decode
    # waits for them.
    w = VrPlan(pat, P, light=True)
    # the caller on the host's least busy 8-CPU group for config 4 (the plan's threads follow it)
    group = quiet_cpu_group()
    saved_aff = None
    if group:
        try:
            saved_aff = os.sched_getaffinity(0)
            os.sched_setaffinity(0, group)
        except OSError:
            group, saved_aff = None, None

    def vr_step():
        w.rerun(pat, P, wait=False)
        cur, _, old, _ = w.encode(pl, frames=frames)
        w.decode(cur, old, out=out4, out_len=ol4)
    for _ in range(3):
        vr_step()
    torch.cuda.synchronize()
    # 4 groups of back-to-back steps (a step's host plan overlaps the previous step's device
    # work), each group timed: the host plan's time varies with where its threads land on a
    # two-socket host, so the figure is the median group's time per step, the mean beside it
    nst = max(5, steps)
    per_step = []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(nst):
            vr_step()
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) / nst)
    dt = float(np.median(per_step))
    dt_mean = float(np.mean(per_step))
    w._load(True)
    t0 = time.perf_counter()
    phases = []
    for _ in range(nst):
        phases.append(w.rerun(pat, P, wait=True).plan_ms)
    plan_s = (time.perf_counter() - t0) / nst
    if saved_aff:
        try:
            os.sched_setaffinity(0, saved_aff)
        except OSError:
            pass
    # device work alone: 50 back-to-back encode + decode pairs (with 5, the final synchronisation's
    # latency stayed in the figure: 0.185 - 0.187 ms in the round profiles against 0.172 ms over 50,
    # profiles/r05/vr/r05zzq_host_probe.log)
    dev_dt = timed(lambda: (v.encode(pl, frames=frames), v.decode(frames[0], frames[2], out=out4, out_len=ol4)),
                   max(50, nst))
    fate = torch.from_numpy(v.fate).cuda()
    ok4 = fate != 3
    res["config4_adaptive"] = {
        "GiB_s": round(P * L / dt / 2**30, 2), "ms": round(dt * 1e3, 3), "packets": P,
        "ms_mean": round(dt_mean * 1e3, 3), "ms_min_max": [round(min(per_step) * 1e3, 3), round(max(per_step) * 1e3, 3)],
        "steps": f"4 groups of {nst}", "instances": int(len(v.encoders)), "switches": v.switches, "coding_rate": round(v.coding_rate, 4),
        "lost": int((ol4 == 0).sum()), "expected_lost": 2982,
        "host_plan_ms": round(plan_s * 1e3, 3),
        "cpu_group": f"{group[0]}-{group[-1]}" if group else None,
        "host_plan_phases_ms": {k: round(sum(p[k] for p in phases) / len(phases), 3) for k in phases[0]},
        "device_only": {"GiB_s": round(P * L / dev_dt / 2**30, 2), "ms": round(dev_dt * 1e3, 3)},
        "note": "ms = one step (the median of 4 timed groups of back-to-back steps): the host plan from scratch (serial control loop: sender, "
                "Variable_Rate_FEC_Encoder, receiver feedback, decoder swaps; the estimator "
                "feedback and the symbolic decoder instances on host threads) + its table "
                "uploads + the device work (one encode launch over every encoder instance of "
                "every (T,B,N), launched after the control loop so that it overlaps the symbolic "
                "decoders; decode = one launch holding the copy tiles and the recovery over the plan's "
                "coefficient rows); host_plan_ms = the plan alone, both phases waited for; "
                "device_only = encode + decode back to back (50 pairs), no plan",
        "verified": bool(torch.equal(out4[ok4], pl[:P][ok4])) and v.lost == 2982 and
        int((ol4 == 0).sum()) == 2982 and w.lost == 2982}
    res["multistream_10k"] = multistream(steps)
    res["relay_10_3"] = relay_chains(steps, kprof)
    res["relay_adaptive"] = relay_adaptive(steps)
    res["relay_session"] = relay_session(steps)
    res["per_packet_api"] = per_packet_api()
    return res


def per_packet_api(packets=20000):
    """The reference's per-packet contract (FEC_Encoder::onTransmit / FEC_Decoder::onReceive, one
    call per seq) from C: tools/stream_latency.cpp built against libfec_amd.so and run as a child
    process, (10,3,3) with bursts of erasures; the reference's own figures are 14.37 us per
    onTransmit and 0.48 us per fast-path onReceive on one core."""
    import re
    import shutil
    import subprocess
    import tempfile
    from fec_erasure_code_unit_test_relay_amd import _lib
    gxx = shutil.which("g++")
    if gxx is None:
        return {"skipped": "no g++"}
    libdir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "stream_latency")
        b = subprocess.run([gxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "stream_latency.cpp"), "-L", libdir, "-lfec_amd",
                            f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True, timeout=120)
        if b.returncode != 0:
            return {"skipped": "build failed: " + b.stderr[-300:]}
        r = subprocess.run([exe, str(packets)], capture_output=True, text=True, timeout=120)
    out = r.stdout
    m = re.search(r"fec_encoder_transmit ([\d.]+) us/call, fec_decoder_receive ([\d.]+) us/call "
                  r"\((\d+) packets, (\d+) erased, (\d+) lost, (\d+) wrong\)", out)
    if r.returncode != 0 or not m:
        return {"skipped": "run failed: " + (r.stderr or out)[-300:]}
    res = {"packets": int(m.group(3)), "erased": int(m.group(4)),
           "onTransmit_us": float(m.group(1)), "onReceive_us": float(m.group(2)),
           "reference_onTransmit_us": 14.37, "reference_onReceive_fast_path_us": 0.48,
           "verified": int(m.group(6)) == 0}
    for key, pat in (("onReceive_received_output", r"output received.*?mean ([\d.]+) p50 ([\d.]+) p99 ([\d.]+)"),
                     ("onReceive_recovered_output", r"output erased.*?mean ([\d.]+) p50 ([\d.]+) p99 ([\d.]+)")):
        q = re.search(pat, out)
        if q:
            res[key] = {"mean_us": float(q.group(1)), "p50_us": float(q.group(2)), "p99_us": float(q.group(3))}
    return res


def relay_type2_setup():
    """The type-2 relay chain's inputs (360 000 source (10,3,3) codewords, hop erasures
    bin/erasure.bin / bin/erasure2.bin) and preallocated outputs."""
    import torch
    from fec_erasure_code_unit_test_relay_amd import Codec, fill_payload
    from fec_erasure_code_unit_test_relay_amd.relay import SymbolWiseRelay
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    P = 360000
    c = Codec(L, 10, 3, 3)
    payload = fill_payload(0, P, L, 0x5EED)
    cw, _ = c.encode(payload)
    e1 = torch.from_numpy(load_pattern("bin_erasure")[:P].astype(np.uint8).copy()).cuda()
    e2 = torch.from_numpy(load_pattern("bin_erasure2")[:P].astype(np.uint8).copy()).cuda()
    r2 = SymbolWiseRelay(L, 10, 3, 10, 3)
    bufs = (torch.empty((P, r2.frame_bytes), dtype=torch.uint8, device="cuda"),
            torch.empty(P, dtype=torch.uint8, device="cuda"),
            torch.empty((P, r2.S * r2.k), dtype=torch.uint8, device="cuda"),
            torch.empty(P, dtype=torch.uint8, device="cuda"))
    return P, c, payload, cw, e1, e2, r2, bufs


def relay_chain_launches(n):
    """rocprofv3 child leg: the type-2 relay and destination kernels, n launches each (after 3)."""
    import torch
    P, c, payload, cw, e1, e2, r2, (fr, rf, dout, dfl) = relay_type2_setup()
    for _ in range(3 + n):
        r2.relay(cw, e1, fr, rf)
        r2.destination(fr, e2, dout, dfl)
    torch.cuda.synchronize()


def relay_chains(steps, kprof=None):
    """The Decoder_Symbol_Wise relay: source (10,3,3) codewords of 360 000 packets
    -> relay -> destination, hop 1 erasures bin/erasure.bin, hop 2 bin/erasure2.bin, for
    RELAYING_TYPE 2 (symbol_wise_encode_1 / decode_1) and 3 (state-dependent).  One step = relay +
    destination of the whole batch; type 3's host planners (the reference's per-packet control
    flow over flags and headers) are inside it.  verified: with clean hops every source packet
    comes out of the destination at the chain's delay."""
    import torch
    from fec_erasure_code_unit_test_relay_amd import Codec, fill_payload
    from fec_erasure_code_unit_test_relay_amd.relay import StateDependentRelay, SymbolWiseRelay
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    P = 360000
    c = Codec(L, 10, 3, 3)
    payload = fill_payload(0, P, L, 0x5EED)
    cw, _ = c.encode(payload)
    e1 = load_pattern("bin_erasure")[:P].astype(np.uint8)
    e2 = load_pattern("bin_erasure2")[:P].astype(np.uint8)
    z = np.zeros(P, dtype=np.uint8)
    res = {"packets": P, "hops": "bin/erasure.bin, bin/erasure2.bin"}
    r2 = SymbolWiseRelay(L, 10, 3, 10, 3)
    e1d, e2d, zd = (torch.from_numpy(x.copy()).cuda() for x in (e1, e2, z))
    o, df = r2.destination(r2.relay(cw, zd)[0], zd)
    D = r2.delay
    ok2 = bool(torch.equal(o[D:, 2:2 + L], payload[:P - D])) and int(df.sum()) == 0
    dt2 = timed(lambda: r2.destination(r2.relay(cw, e1d)[0], e2d), steps)
    res["type2"] = {"ms": round(dt2 * 1e3, 3), "GiB_s": round(P * L / dt2 / 2**30, 2), "verified": ok2}
    # roofline of the two type-2 kernels (fec_sw_fast_relay_kernel / fec_sw_fast_dest_kernel): an event
    # pair around each launch on its stream, outputs preallocated; algorithmic bytes per packet =
    # relay: CW + 1 flag read, frame + 1 flag written; destination: frame + 1 flag read, S*k + 1 written
    fr = torch.empty((P, r2.frame_bytes), dtype=torch.uint8, device="cuda")
    rf = torch.empty(P, dtype=torch.uint8, device="cuda")
    dout = torch.empty((P, r2.S * r2.k), dtype=torch.uint8, device="cuda")
    dfl = torch.empty(P, dtype=torch.uint8, device="cuda")

    def ev_ms(fn, n=20):
        for _ in range(3):
            fn()
        tot = 0.0
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / n
    ms_r = ev_ms(lambda: r2.relay(cw, e1d, fr, rf))
    ms_d = ev_ms(lambda: r2.destination(fr, e2d, dout, dfl))
    by_r = (c.CW + 1 + r2.frame_bytes + 1) * P
    by_d = (r2.frame_bytes + 1 + r2.S * r2.k + 1) * P
    res["type2"]["roofline"] = {
        "bound": "hbm", "peak": 8000.0, "unit": "GB/s",
        "relay": {"us": round(ms_r * 1e3, 1), "bytes": by_r, "achieved": round(by_r / ms_r / 1e6, 1),
                  "frac": round(by_r / ms_r / 1e6 / 8000.0, 4)},
        "destination": {"us": round(ms_d * 1e3, 1), "bytes": by_d, "achieved": round(by_d / ms_d / 1e6, 1),
                        "frac": round(by_d / ms_d / 1e6 / 8000.0, 4)},
        "note": "per kernel: algorithmic bytes / kernel time; relay CW+1 read + frame+1 written, destination "
                "frame+1 read + S*k+1 written per packet.  us / frac: this invocation's rocprofv3 child "
                "(the relay and destination launched 20 times after the headline step) when it ran, else the "
                "event pair around each launch on its stream (us_event / frac_event beside it); traffic: the "
                "committed FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes of tools/swdf_bench.py when they were "
                "made on these kernel sources"}
    for leg, prefix in (("relay", "fec_sw_fast_relay"), ("destination", "fec_sw_fast_dest")):
        d = res["type2"]["roofline"][leg]
        d.update(us_event=d["us"], frac_event=d["frac"])
        names = [k for k in ((kprof or {}).get("__all__") or {}) if k.startswith(prefix)]
        if names:
            k = max(names, key=lambda n: kprof["__all__"][n]["calls"])
            us = kprof["__all__"][k]["avg_us"]
            d.update(kernel=k, us=round(us, 1), achieved=round(d["bytes"] / us / 1e3, 1),
                     frac=round(d["bytes"] / us / 1e3 / 8000.0, 4), us_source="rocprofv3 child of this bench",
                     rocprof_calls=kprof["__all__"][k]["calls"])
            tr = pmc_traffic(k)
            if tr and tr[2]:
                d.update(traffic=tr[0], traffic_ratio=round(tr[0] / d["bytes"], 3), traffic_source=tr[1])
            elif tr:
                d.update(traffic=None, traffic_stale=f"{tr[1]} was measured on other kernel sources")
    r3 = StateDependentRelay(L, 10, 3, 10, 3)
    o, df = r3.destination(r3.relay(cw, z), z)
    D = r3.delay
    ok3 = bool(torch.equal(o[D:, 2:2 + L], payload[:P - D])) and int(df.sum()) == 0
    dt3 = timed(lambda: r3.destination(r3.relay(cw, e1), e2), max(1, min(steps, 2)))
    res["type3"] = {"ms": round(dt3 * 1e3, 3), "GiB_s": round(P * L / dt3 / 2**30, 3), "verified": ok3,
                    "note": "host planners included (relay and destination control flow per packet)"}
    return res


def relay_adaptive(steps):
    """The relay chain under variable rate (Variable_Rate_FEC_Decoder.cpp:600-740, :1423-1600,
    :1772-1873): config 4's code switches on bin/erasure.bin as the source schedule, hop 1
    bin/erasure.bin, hop 2 bin/erasure2.bin, 360 000 seqs, RELAYING_TYPE 2 and 3.  One step = the
    whole chain (per code instance a fresh source encoder, relay and destination; double coding
    at every switch; frames and reported outputs gathered to seq order), type 3's host planners
    inside.  verified: the per-100-seq digests of every frame, output and flag equal the
    reference-structured driver's over the oracle methods (tests/golden/relay_vr_360k.json)."""
    import json
    import torch
    from fec_erasure_code_unit_test_relay_amd import fill_payload
    from fec_erasure_code_unit_test_relay_amd.relay import AdaptiveRelay, relay_digest
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden",
                                    "relay_vr_360k.json")))
    P = g["P"]
    payload = fill_payload(0, P, L, 0x5EED)
    e1, e2 = load_pattern("bin_erasure")[:P], load_pattern("bin_erasure2")[:P]
    res = {"packets": P, "codes": len(g["schedule"]), "hops": "bin/erasure.bin, bin/erasure2.bin"}
    for t in (2, 3):
        r = AdaptiveRelay(t, L, g["schedule"], P)
        frames, flen, out, flags = r.run(payload, e1, e2)
        torch.cuda.synchronize()
        ok = [f"{c:08x}" for c in relay_digest(frames, flen, out, flags)] == g[f"type{t}"]["blocks"]
        dt = timed(lambda: r.run(payload, e1, e2), max(1, min(steps, 3)))
        res[f"type{t}"] = {"ms": round(dt * 1e3, 3), "GiB_s": round(P * L / dt / 2**30, 3),
                           "unflagged": int((flags == 0).sum()), "verified": bool(ok)}
    res["note"] = ("one fixed-rate batch per code over its instances laid end to end (each behind zero rows), "
                   "planners reset per instance; type 2's erasure rows and flags gathered on the device, type 3's "
                   "host planners (and their erasure rows) inside; "
                   "verified = equal to tests/golden/relay_vr_360k.json, made by this repo's reference-structured "
                   "driver over the oracle's methods (the reference ships no relay output: parity unpinned)")
    return res


def relay_session(steps):
    """The two-hop adaptive relay session (RELAYING_TYPE 2 and 3 with N_INITIAL = N_INITIAL_2 = -1,
    application_local_simulation.cpp:71-593): the source splits T_TOT over the hops from the relay's
    12-byte feedback, the relay re-encodes symbol-wise, the destination decodes; hop 1
    bin/erasure.bin, hop 2 bin/erasure2.bin, Q = 360 020 seqs (the reference's loop to seq
    NUMBER_OF_ITERATIONS + T + T2 - 1).  control_ms: the host control plane from scratch (the
    session's every decision, symbolic); ms: one run of the session's byte work on the GPU (the
    source's encoder instances, every relay call's symbols, the relay lineages, the destination's
    outputs and loss check).  verified: the lost count and the control plane's totals equal the
    oracle's committed run (tests/golden/relay_session_360k.json)."""
    import json
    import torch
    from fec_erasure_code_unit_test_relay_amd import fill_payload
    from fec_erasure_code_unit_test_relay_amd.relay import RelaySession
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden",
                                    "relay_session_360k.json")))
    Q = g["Q"]
    e1, e2 = load_pattern("bin_erasure"), load_pattern("bin_erasure2")
    payload = fill_payload(0, Q, L, 0x5EED)
    res = {"seqs": Q, "hops": "bin/erasure.bin, bin/erasure2.bin"}
    for t in (2, 3):
        t0 = time.perf_counter()
        s = RelaySession(t, Q, e1, e2)
        ctl = time.perf_counter() - t0
        relay, out, lost, count = s.run(payload)
        torch.cuda.synchronize()
        dt = timed(lambda: s.run(payload, relay, out, lost, count), max(3, min(steps, 10)))
        ref = g["types"][str(t)]
        st = s.stats
        ok = int(count.item()) == ref["lost"] and st["relay_bytes"] == ref["relay_bytes"] and \
            st["src_switches"] == ref["src_switches"] and st["rate2"] == ref["rate2_sum"]
        res[f"type{t}"] = {"ms": round(dt * 1e3, 3), "GiB_s": round(Q * L / dt / 2**30, 3),
                           "control_ms": round(ctl * 1e3, 1), "lost": int(count.item()),
                           "switches": st["src_switches"], "relay_calls": st["relay_calls"],
                           "lineages": st["lineages"], "longest_lineage": st["longest_lineage"],
                           "rate_first_hop": round(st["rate1"] / st["rate1_n"], 4),
                           "rate_second_hop": round(st["rate2"] / st["rate2_n"], 4),
                           "oracle_seconds_1_core": ref["oracle_seconds"], "verified": bool(ok)}
    return res


def multistream(steps, NS=10000):
    """Many independent streams (north_star: "many independent (T,B,N) coding windows batched
    across wavefronts"): 10 000 streams at (10,3,3), one call = the next packet of every stream
    (fec_streams_encode then fec_streams_decode, one launch each; the decoders' symbolic steps on
    the host are inside the timed region).  Stream s sees bin/erasure.bin from phase 36*s."""
    import torch
    from fec_erasure_code_unit_test_relay_amd import StreamGroup, fill_payload
    from fec_erasure_code_unit_test_relay_amd.streams import load_pattern
    T = 10
    base = load_pattern("bin_erasure")[:360000]
    grp = StreamGroup(L, T, 3, 3, NS)
    ids = np.arange(NS, dtype=np.int32)
    warm, rounds = 12, max(20, steps)
    R = warm + rounds
    pays = fill_payload(0, R * NS, L, 0xA11).view(R, NS, L)
    ph = (36 * ids.astype(np.int64)) % base.size
    ers = np.stack([base[(ph + r) % base.size] for r in range(R)]).astype(np.uint8)
    cw = torch.empty((NS, grp.CW), dtype=torch.uint8, device="cuda")
    wl = torch.empty(NS, dtype=torch.int32, device="cuda")
    out = torch.empty((R, NS, L), dtype=torch.uint8, device="cuda")
    ol = torch.empty((R, NS), dtype=torch.int32, device="cuda")

    def call(r):
        grp.encode(ids, pays[r], out=cw, out_len=wl)
        grp.decode(ids, ers[r], cw, out=out[r], out_len=ol[r])
    for r in range(warm):
        call(r)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(warm, R):
        call(r)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / rounds
    # encode alone (the same streams keep going: later packets)
    t0 = time.perf_counter()
    for r in range(warm, R):
        grp.encode(ids, pays[r], out=cw, out_len=wl)
    torch.cuda.synchronize()
    dte = (time.perf_counter() - t0) / rounds
    # check: the output of round r is packet r-T of each stream (sent in round r-T); every
    # delivered row equals its source, and none is missing where the pattern lost nothing near it
    ok = True
    for r in range(warm, R):
        d = ol[r] == L
        ok = ok and bool(torch.equal(out[r][d], pays[r - T][d])) and int((ol[r] != 0).sum()) >= int(d.sum())
    return {"streams": NS, "packets_per_call": NS, "calls": rounds,
            "us_per_call": round(dt * 1e6, 1), "us_per_packet": round(dt * 1e6 / NS, 4),
            "encode_us_per_packet": round(dte * 1e6 / NS, 4),
            "reference_cpu_encode_us_per_packet": 14.37,
            "GiB_s": round(NS * L / dt / 2**30, 3),
            "note": "one call = encode + decode of the next packet of every stream, host symbolic "
                    "decoder steps included; reference figure: SURVEY.md section 6 (1 core, ISA-L)",
            "verified": ok}


def launch_mode(gpus: int, env) -> str:
    """How this process takes part in a --gpus N run.

    'spawn': no WORLD_SIZE in the environment and N > 1 -- this process is the launcher; it starts N
    rank processes (spawn_ranks) and never touches the GPU itself.  'run': it is a rank (WORLD_SIZE
    set by torchrun or by spawn_ranks, or N == 1).  A WORLD_SIZE that disagrees with --gpus is an
    error: the JSON line would report a different n_gpus than the one asked for."""
    if gpus < 1:
        raise SystemExit(f"bench.py: --gpus must be >= 1 (got {gpus})")
    ws = env.get("WORLD_SIZE")
    if ws is None or ws == "":
        return "spawn" if gpus > 1 else "run"
    if int(ws) != gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={ws} but --gpus {gpus}: launch {gpus} ranks "
                         f"(torchrun --nproc-per-node {gpus}) or drop WORLD_SIZE")
    return "run"


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv) -> int:
    """Start n rank processes of this script (one per GPU: RANK = LOCAL_RANK = r, WORLD_SIZE = n,
    rendezvous on 127.0.0.1) and wait for them.  The launcher never initialises the GPU, so the
    ranks are fresh processes, not forks or execs of a GPU process.  If a rank fails, the others
    (which would wait forever in a collective) are terminated; the exit code is the first failing
    rank's, else 0.  Rank 0 prints the JSON line on the inherited stdout."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 128 - code
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc


def launch_selftest(world: int, rank: int) -> None:
    """--launch-selftest: the rank side of spawn_ranks without a GPU (CPU test of the launcher):
    gloo rendezvous, one all-reduce of the ranks, rank 0 prints what it saw."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group(backend="gloo")
    t = torch.tensor([rank, 1], dtype=torch.int64)
    if world > 1:
        dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"n_gpus": world, "rank_sum": int(t[0]), "ranks": int(t[1]),
                          "master": os.environ.get("MASTER_ADDR")}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--packets", type=int, default=1_000_000, help="decoded packets per GPU")
    ap.add_argument("--tbn", default="10,3,3")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also check the timed work and measure everything else "
                         "(per-kernel times and roofline, host-inclusive rates, configs 3 and 4, relay and "
                         "multi-stream legs, CPU baseline); the --no-* options below trim a --full run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--stream-id", type=int, default=None,
                    help="payload seed and pattern phase of this stream (default: the rank); a single-rank "
                         "run with --stream-id r reproduces rank r's stream of a multi-rank run")
    ap.add_argument("--cpu-packets", type=int, default=30000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-inclusive", action="store_true")
    ap.add_argument("--encode-path", default="auto", help="A/B: auto|generic|tile")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip BASELINE configs 3 and 4")
    ap.add_argument("--warm-seconds", type=float, default=1.0,
                    help="untimed replays of the step for this much wall time before the W warm-up "
                         "steps: a fresh box's clocks (and the new buffers) need >100 steps to settle "
                         "(20 timed steps after 5 warm-up: 0.400 ms/step, after 100: 0.355)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as a captured hipGraph instead of launching its kernels one by one")
    ap.add_argument("--no-graph", action="store_true", help="(the default) eager launches")
    ap.add_argument("--pipeline", action="store_true",
                    help="overlap batch i's recovery pass with batch i+1's encode (codewords and "
                         "decoder workspaces double-buffered; the copy and the recovery write "
                         "disjoint output rows)")
    ap.add_argument("--launch-selftest", action="store_true",
                    help="CPU test of the --gpus launcher: ranks rendezvous over gloo, no GPU work")
    ap.add_argument("--rocprof-child", action="store_true",
                    help="(internal) the step alone under rocprofv3, started by this bench for its roofline")
    ap.add_argument("--no-rocprof", action="store_true",
                    help="take the roofline's kernel time from HIP events only (no rocprofv3 child run)")
    ap.add_argument("--rocprof-keep", default=None,
                    help="keep the rocprofv3 child's output (kernel_stats.csv) in this directory")
    args = ap.parse_args()
    T, B, N = map(int, args.tbn.split(","))
    # The library's run-time settings in effect are recorded in the line (`env`); a setting that
    # skips work cannot produce a valid line (the product library compiles the encoder's ablation
    # switch out, but a diagnostic build might be loaded).
    fec_env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("FEC_")}
    if fec_env.get("FEC_TILE_DBG", "0") not in ("", "0"):
        raise SystemExit("bench.py: FEC_TILE_DBG (work-skipping encoder ablation) is set; refusing to measure")

    if launch_mode(args.gpus, os.environ) == "spawn":
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launch_selftest:
        launch_selftest(world, rank)
        return

    import torch
    import torch.distributed as dist

    # FEC_BENCH_BACKEND=gloo rehearses the multi-rank bench on a box with fewer GPUs than ranks
    # (ranks share devices round-robin, collectives on host tensors); the driver's runs use RCCL.
    backend = os.environ.get("FEC_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend != "nccl":
        local = local % max(1, ndev)
    elif local >= ndev:
        raise SystemExit(f"bench.py: rank {rank} has LOCAL_RANK {local} but only {ndev} GPUs are "
                         f"visible (set FEC_BENCH_BACKEND=gloo to rehearse ranks on shared GPUs)")
    torch.cuda.set_device(local)
    comm_dev = "cuda" if backend == "nccl" else "cpu"
    if world > 1:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)

    from fec_erasure_code_unit_test_relay_amd import Codec, fill_payload

    P = args.packets
    Pf = P + T  # fed packets: the last T only complete the outputs of packets P-T..P-1
    codec = Codec(L, T, B, N)
    if args.encode_path != "auto":
        codec.set_encode_path(args.encode_path)
    sid = rank if args.stream_id is None else args.stream_id + rank
    seed = stream_seed(sid)
    pat = stream_pattern(Pf, sid)
    payload = fill_payload(0, Pf, L, seed)
    er = torch.from_numpy(pat).cuda()
    cw = torch.empty((Pf, codec.CW), dtype=torch.uint8, device="cuda")
    wl = torch.empty(Pf, dtype=torch.int32, device="cuda")
    out = torch.empty((P, L), dtype=torch.uint8, device="cuda")
    ol = torch.empty(P, dtype=torch.int32, device="cuda")
    codec.workspace(Pf)

    def step():
        # encode the batch, then decode it (fec_decode_batch: the erasure-only plan runs on the
        # codec's side stream beside the received-packet copy, joined before the recovery pass).
        # The plan is not started beside the encoder: the encoder leaves wave slots free on
        # purpose (fec_codec.hip, launch_encode_wave), and planner kernels there cost it ~45 us.
        codec.encode(payload, out=cw, out_len=wl)
        codec.decode(cw, er, out=out, out_len=ol)

    # --pipeline: step i = encode into codeword buffer i%2; plan (codec i%2's workspace, on its side
    # stream, after the encode) beside the received-packet copy; the recovery of batch i on a third
    # stream after both, so that it runs beside batch i+1's encode.  Batch i+2 reuses buffer i%2
    # only after batch i's recovery.  Every step still encodes and decodes the whole batch; the
    # timed region ends with a device synchronisation, after the last recovery.
    codecs, cws, wls = [codec], [cw], [wl]
    if args.pipeline:
        codecs.append(Codec(L, T, B, N))
        codecs[1].workspace(Pf)
        cws.append(torch.empty_like(cw))
        wls.append(torch.empty_like(wl))
        plan_streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        rec_stream = torch.cuda.Stream()
        rec_done = [torch.cuda.Event(), torch.cuda.Event()]
        pstate = {"i": 0}

        def pstep():
            b = pstate["i"] & 1
            pstate["i"] += 1
            c = codecs[b]
            main = torch.cuda.current_stream()
            main.wait_event(rec_done[b])  # batch i-2's recovery read cws[b] and workspace b
            c.encode(payload, out=cws[b], out_len=wls[b])
            enc_done = torch.cuda.Event()
            enc_done.record(main)
            ps = plan_streams[b]
            ps.wait_event(enc_done)
            with torch.cuda.stream(ps):
                c.plan(er, Pf)
            plan_done = torch.cuda.Event()
            plan_done.record(ps)
            c.copy(cws[b], er, out=out, out_len=ol)
            copy_done = torch.cuda.Event()
            copy_done.record(main)
            rec_stream.wait_event(copy_done)
            rec_stream.wait_event(plan_done)
            with torch.cuda.stream(rec_stream):
                c.recover(cws[b], out, ol)
            rec_done[b].record(rec_stream)
        step = pstep  # noqa: F811

    def barrier():
        if world > 1:
            dist.barrier()

    # The step (encode; fork; plan on the codec's side stream | copy; join; recover: 6 kernels and
    # 3 memsets) is launched eagerly: the kernels queue ahead of the GPU, and on a replayed hipGraph
    # of the same step the copy waits for the side stream's first memset and the recovery starts
    # later after the copy (0.3208 / 0.3210 / 0.3199 ms graph vs 0.3159 / 0.3127 / 0.3145 ms eager
    # at 20 / 20 / 100 steps, alternating processes on one box: tools/graph_ab.sh,
    # profiles/r03/r03y_graph_ab.txt).  --graph replays the captured step instead.
    run = step
    if args.graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        run = graph.replay

    warm_steps = 0
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < args.warm_seconds:
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        warm_steps += 10
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    t_submit = time.perf_counter() - t0  # host time to enqueue the K steps (diagnostic)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed, dist, comm_dev)
    if args.rocprof_child:  # the profiled child: the step's kernels, then the type-2 relay chain's
        print(json.dumps({"rocprof_child": True, "ms_per_step": elapsed / args.steps * 1e3}), flush=True)
        if world == 1 and not args.no_extra_configs:
            relay_chain_launches(20)
        return

    if args.dump_outputs:  # the last timed step's buffers (--pipeline: the codewords it wrote last)
        last = (pstate["i"] - 1) % len(cws) if args.pipeline else 0
        dump_outputs(args.dump_outputs, cws[last], wls[last], out, ol, f"_rank{rank}" if rank else "")

    if not args.full:  # the plain run: the headline line alone
        if rank == 0:
            print(json.dumps({
                "metric": "GiB/s device-resident erasure encode+decode, 300B pkts, T=10; %HBM roofline",
                "value": round(world * P * L / (elapsed / args.steps) / 2**30, 3),
                "unit": "GiB/s",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "u8",
                "config": {"workload": f"encode {Pf} + decode {P} x 300B packets per GPU, one stream "
                                       f"per GPU, (T,B,N)=({T},{B},{N})",
                           "T": T, "B": B, "N": N, "packets_per_gpu": P},
                "env": fec_env,
                "host_submit_ms_per_step": round(t_submit / args.steps * 1e3, 4),
                "step_launch": ("hipGraph replay" if args.graph else "eager launches") +
                               ("; batch i's recovery beside batch i+1's encode (--pipeline)" if args.pipeline else ""),
                "device_warmup": {"seconds": args.warm_seconds, "untimed_steps": warm_steps},
                "full": False}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # correctness of the timed work (outside the timed region): round trip + planner agreement
    eps, rec, lost = codec.counters()
    lost_mask = (ol == 0)
    ok_rows = ~lost_mask
    verified = bool(torch.equal(out[ok_rows], payload[:P][ok_rows])) and \
        int((ol[ok_rows] != L).sum()) == 0 and int(lost_mask.sum()) == lost
    # trivial counter reduction over RCCL
    rec_all, lost_all, erased_all, verified_all = reduce_counters(
        [rec, lost, int(pat[:P].sum()), int(verified)], dist, comm_dev)
    # every rank's own counters and an output digest (the test compares them with single-rank runs
    # of the same stream, --stream-id)
    digest = int(torch.sum(ol.to(torch.int64) * torch.arange(1, P + 1, device=ol.device, dtype=torch.int64)).item())
    mine = torch.tensor([sid, int(pat[:P].sum()), rec, lost, int(verified), digest], dtype=torch.int64,
                        device=comm_dev)
    if world > 1:
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
    else:
        allr = [mine]
    per_rank = [dict(zip(("stream", "erased", "recovered", "lost", "verified", "out_len_digest"),
                         (int(x) for x in t.tolist()))) for t in allr]

    # per-kernel durations: HIP events on the launch stream, separate pass
    # (warm-up launches first, so the averages are the steady state the rocprofv3 trace sees)
    for _ in range(5):
        step()
    for c in codecs:
        c.timing(True)
    for _ in range(50):
        step()
    kt = {}
    for c in codecs:
        for k, (ms, n) in c.collect_timing().items():
            t0_, n0_ = kt.get(k, (0.0, 0))
            kt[k] = (t0_ + ms, n0_ + n)
        c.timing(False)
    per_launch = {k: (ms / n if n else 0.0) for k, (ms, n) in kt.items()}

    # The two byte kernels alone, launched back to back 50 times between two HIP events on their
    # launch stream (torch's current stream): reported beside the in-step durations.
    def back_to_back(fn, n=50):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    b2b = {"fec_encode_kernel": back_to_back(lambda: codec.encode(payload, out=cw, out_len=wl)),
           "fec_copy_kernel": back_to_back(lambda: codec.copy(cw, er, out=out, out_len=ol))}
    algo = {"fec_encode_kernel": (L + codec.CW) * Pf, "fec_copy_kernel": (codec.CW + 1 + L) * P}
    # The event figure's duration is the in-step one (the event pair bound to each launch of the
    # step's kernels, above): the kernel in the context it is timed in; the kernel alone back to
    # back is slower than in the step (the copy's non-temporal traffic leaves the caches to the
    # encoder there).
    dominant = max(algo, key=lambda k: per_launch[k])
    achieved = algo[dominant] / (per_launch[dominant] * 1e-3) / 1e9

    result = None
    kt_all = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = world * P * L / (elapsed / args.steps) / 2**30
        result = {
            "metric": "GiB/s device-resident erasure encode+decode, 300B pkts, T=10; %HBM roofline",
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic payloads (splitmix64, seed per GPU); erasures = bin/erasure.bin "
                    "(reference recording) replayed, phase per GPU",
            "config": {"workload": f"encode {Pf} + decode {P} x 300B packets per GPU, one stream "
                                   f"per GPU, (T,B,N)=({T},{B},{N})",
                       "T": T, "B": B, "N": N, "k": codec.k, "n": codec.n, "S": codec.S,
                       "codeword_bytes": codec.CW, "packets_per_gpu": P,
                       "parallelism": f"streams{world} (one independent stream per GPU)"},
            "verified": bool(verified_all == world),
            "env": fec_env,
            "host_submit_ms_per_step": round(t_submit / args.steps * 1e3, 4),
            "step_launch": ("hipGraph replay" if args.graph else "eager launches") +
                           ("; batch i's recovery beside batch i+1's encode (--pipeline)" if args.pipeline else ""),
            "device_warmup": {"seconds": args.warm_seconds, "untimed_steps": warm_steps,
                              "note": "untimed replays of the same step before the W warm-up steps "
                                      "(clock / first-touch settling); the timed K steps are unchanged"},
            "decode": {"erased": erased_all, "recovered": rec_all, "lost": lost_all},
            "per_rank": per_rank,
            "algorithmic_bytes_per_packet": L + codec.CW + codec.CW + 1 + L,
            "algorithmic_GBps": round(world * P * (2 * L + 2 * codec.CW + 1) / (elapsed / args.steps) / 1e9, 1),
            "kernels_ms_per_launch": {k: round(v, 5) for k, v in per_launch.items()},
            "kernels_ms_back_to_back": {k: round(v, 5) for k, v in b2b.items()},
            "roofline": {"bound": "hbm", "kernel": dominant, "achieved": round(achieved, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None},
        }
        info = codec.info()
        symbol = info["encode_kernel"] if dominant == "fec_encode_kernel" else info.get("copy_kernel")
        result["roofline"].update(algorithmic_bytes=algo[dominant])
        # The kernel time of the roofline: this invocation's own rocprofv3 trace of the same step
        # (a child process of this bench, on this box, on these sources), dominant kernel = the
        # slower of the two byte kernels by it; the HIP-event figure (events bound to each launch,
        # hipExtLaunchKernel) is reported beside it.  --no-rocprof: the event figure alone.
        rf = result["roofline"]
        rf.update(achieved_event=rf["achieved"], frac_event=rf["frac"], kernel_event=dominant)
        sym = {"fec_encode_kernel": info["encode_kernel"], "fec_copy_kernel": info.get("copy_kernel")}
        kt, kinfo = (None, "--no-rocprof") if args.no_rocprof or P != 1_000_000 else rocprof_child(
            [a for a in sys.argv[1:] if a not in ("--rocprof-child",)], list(sym.values()), args.rocprof_keep)
        kt_all = kt
        if kt and all(v in kt for v in sym.values() if v):
            dom = max((k for k in sym if sym[k]), key=lambda k: kt[sym[k]]["avg_us"])
            a_rp = algo[dom] / (kt[sym[dom]]["avg_us"] * 1e-6) / 1e9
            rf.update(kernel=dom, achieved=round(a_rp, 1), frac=round(a_rp / HBM_PEAK_GBS, 4),
                      algorithmic_bytes=algo[dom], rocprof_avg_us=round(kt[sym[dom]]["avg_us"], 2),
                      frac_source="rocprofv3 --kernel-trace --stats of this bench's step, run by this "
                                  "invocation as a child process (" + kinfo + ")",
                      rocprof_kernels_us={k: round(kt[v]["avg_us"], 2) for k, v in sym.items() if v},
                      rocprof_calls={k: kt[v]["calls"] for k, v in sym.items() if v})
            symbol = sym[dom]
        else:
            rf.update(frac_source="HIP events bound to each launch (rocprofv3 child: " + str(kinfo) + ")")
        # HBM traffic per launch from the committed FETCH_SIZE / WRITE_SIZE passes of this command,
        # only when they were measured on the current sources
        tr = pmc_traffic(symbol) if symbol and P == 1_000_000 else None
        rf.update(traffic=None, traffic_kernel=symbol)
        if tr and tr[2]:
            rf.update(traffic=tr[0], traffic_unit="bytes per launch", traffic_source=tr[1])
        elif tr:
            rf.update(traffic_stale=f"{tr[1]} was measured on other kernel sources")
    if not args.no_host_inclusive:
        hi = host_inclusive(codec, payload, pat, er, cw, wl, out, ol, P, Pf, world, barrier,
                            lambda x: max_over_ranks(x, dist, comm_dev),
                            lambda v: reduce_counters(v, dist, comm_dev))
        if rank == 0:
            result["host_inclusive"] = hi
    if rank == 0 and world == 1 and not args.no_extra_configs:
        result["configs"] = extra_configs(kprof=kt_all)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(T, B, N, args.cpu_packets, pat)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
