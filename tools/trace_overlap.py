"""Do the kernels of two calls in flight run side by side?  Reads the kernel trace of one bench.py run
(rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py) and prints, for the library's kernels: the queues
they ran on, the time they cover against the sum of their durations, how many of them started while an earlier one was still
running, and the same for k_seed alone -- a step's first kernel: started under the step before, or behind it.
usage: python3 tools/trace_overlap.py DIR"""
import csv
import glob
import os
import sys


def main(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % d)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if "gat::" not in name:
                continue
            short = name.split("gat::")[1].split("(")[0].split("<")[0]
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short, r.get("Queue_Id", "?")))
    rows.sort()
    n = len(rows)
    total = sum(e - s for s, e, _, _ in rows)
    covered, overlapped, seeds, seeds_under, last_end = 0, 0, 0, 0, 0
    per = {}
    for s, e, k, _ in rows:
        under = s < last_end
        overlapped += under
        if k == "k_seed":
            seeds += 1
            seeds_under += under
        covered += max(0, e - max(s, last_end))
        last_end = max(last_end, e)
        c = per.setdefault(k, [0, 0, 0])
        c[0] += 1
        c[1] += e - s
        c[2] += under
    print("kernels of the library        : %d on queues %s" % (n, sorted(set(q for _, _, _, q in rows))))
    print("sum of their durations        : %.3f ms" % (total / 1e6))
    print("time they cover               : %.3f ms (%.1f %% of the sum)" % (covered / 1e6, 100.0 * covered / max(1, total)))
    print("started under an earlier one  : %d of %d" % (overlapped, n))
    print("k_seed (a step's first kernel): %d of %d started while a kernel of the step before was running" % (seeds_under, seeds))
    print("%-24s %6s %10s %8s" % ("kernel", "calls", "avg us", "under"))
    for k, (c, t, u) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        print("%-24s %6d %10.1f %8d" % (k, c, t / c / 1e3, u))


if __name__ == "__main__":
    main(sys.argv[1])
