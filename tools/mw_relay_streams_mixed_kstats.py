"""The message-wise relay kernels' rows of a rocprofv3 kernel trace of tools/mw_relay_streams_mixed_ab.py 5
(3 warm-up and 5 timed rounds per workload), grouped by kernel and workload in the tool's launch order: per
workload the kernel time per round (the sum over the leg's launches) as median, min and max, and per pair
of a one-code leg its launch's median.  Also writes those trace rows alone.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/mw_relay_streams_mixed_ab.py 5
  python tools/mw_relay_streams_mixed_kstats.py DIR/.../run_kernel_trace.csv rows_out.csv > kernel_stats.txt"""
import csv
import statistics as st
import sys

path, out_rows = sys.argv[1], sys.argv[2]
rows = [r for r in csv.DictReader(open(path)) if "fec_mw_relay_streams" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
with open(out_rows, "w", newline="") as f:
    w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
    w.writeheader()
    w.writerows(rows)
REP = 8  # 3 warm-up + 5 repeats
plan = {"mixed": [("(a) five pairs, Q = 1", 1), ("(a) five pairs, Q = 16", 1), ("(a4) three pairs, Q = 1", 1),
                  ("(a4) three pairs, Q = 16", 1), ("(c2) one pair, Q = 16", 1)],
        "plain": [("(b) five groups, Q = 1", 5), ("(b) five groups, Q = 16", 5), ("(b4) three groups, Q = 1", 3),
                  ("(b4) three groups, Q = 16", 3), ("(c1) one group, Q = 16", 1)]}
for kind in ("mixed", "plain"):
    sel = [r for r in rows if ("mixed_kernel" in r["Kernel_Name"]) == (kind == "mixed")]
    name = "fec_mw_relay_streams_mixed_kernel" if kind == "mixed" else "fec_mw_relay_streams_kernel"
    regs = sorted({(r["VGPR_Count"], r["SGPR_Count"], r["Scratch_Size"]) for r in sel})
    print(f"{name}: {len(sel)} launches; (VGPRs, SGPRs, scratch) as traced: {regs}")
    i = 0
    for label, per in plan[kind]:
        blk = sel[i:i + per * REP]
        i += per * REP
        if not blk:
            continue
        # per round: the sum over the leg's launches (launch j of a round is pair j)
        rounds = [blk[j * per:(j + 1) * per] for j in range(len(blk) // per)]
        tot = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rd) / 1e3 for rd in rounds]
        wgs = sum(int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) for r in rounds[0])
        print(f"  {label:28s} {len(blk):3d} launches, {wgs:6d} workgroups per round: kernel time per round median "
              f"{st.median(tot):9.1f} us (min {min(tot):.1f} .. max {max(tot):.1f})")
        if per > 1:
            for j in range(per):
                d = [(int(rd[j]["End_Timestamp"]) - int(rd[j]["Start_Timestamp"])) / 1e3 for rd in rounds]
                print(f"      pair {j}: {int(rounds[0][j]['Grid_Size_X']) // 256:6d} workgroups, median {st.median(d):8.1f} us")
