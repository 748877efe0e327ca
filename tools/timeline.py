#!/usr/bin/env python3
"""Timeline of one pipeline step from a rocprofv3 --kernel-trace CSV: kernel, queue, start, end, duration (us).
usage: python tools/timeline.py s_kernel_trace.csv [step index]

       python tools/timeline.py --summary STEPS s_kernel_trace.csv [out.json]
Summary of the last STEPS steps of a trace of back-to-back runs of a batch that goes down the pipeline as two halves (two
match launches per step), e.g. `rocprofv3 --kernel-trace --output-format csv -- python bench.py --gpus 1 --steps 12 --warmup 2`
with STEPS = 12: the window from the first of their match launches to the end of the last pipeline kernel, and in it
  no_throughput_kernel_resident_*        time during which none of pre-screen, dense count and match is resident
  throughput_overlap_between_lanes_share of the time a throughput kernel is resident, the part in which throughput kernels of
                                         BOTH queues are (lanes that share the chip: lock-step)
  tail_under_other_lane_share            of the resident time of every other pipeline kernel, the part during which a
                                         throughput kernel of the OTHER queue is resident (tails hidden under the other lane)
  kernel_ms_per_step                     resident time (start to end) per kernel name.  Under two lanes a kernel that shares
                                         the chip, or waits for compute units behind the other lane's kernel, is resident for
                                         longer than it runs alone: these sums compare arrangements, not kernels."""
import collections
import csv
import json
import sys

THROUGHPUT = ("ransac_prescreen_kernel", "ransac_count_mfma_kernel", "match_mfma_kernel")


def load(path):
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    rows.sort(key=lambda r: r["s"])
    return rows


def short(name):
    return name.replace("void mvs::", "").replace("mvs::", "").split("(")[0]


def union(iv):
    """sorted, merged intervals"""
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def length(iv):
    return sum(e - s for s, e in iv)


def intersect(a, b):
    """intersection of two merged interval lists"""
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        s, e = max(a[i][0], b[j][0]), min(a[i][1], b[j][1])
        if s < e:
            out.append([s, e])
        if a[i][1] < b[j][1]:
            i += 1
        else:
            j += 1
    return out


def summary(path, steps):
    rows = load(path)
    heavy = lambda r: any(k in r["Kernel_Name"] for k in THROUGHPUT)
    mm = [r for r in rows if "match_mfma" in r["Kernel_Name"]]
    if len(mm) < 2 * steps:
        raise SystemExit("%s: %d match launches, fewer than two per step for %d steps" % (path, len(mm), steps))
    t0 = mm[-2 * steps]["s"]
    pipe = [r for r in rows if r["s"] >= t0 and "mvs::" in r["Kernel_Name"]]
    t1 = max(r["e"] for r in pipe)
    queues = sorted({r["Queue_Id"] for r in pipe})
    hv = {q: union((r["s"], r["e"]) for r in pipe if heavy(r) and r["Queue_Id"] == q) for q in queues}
    hv_all = union(iv for q in queues for iv in hv[q])
    both = []
    for i, q in enumerate(queues):
        for p in queues[i + 1:]:
            both += intersect(hv[q], hv[p])
    tail_total = tail_hidden = 0
    for r in pipe:
        if heavy(r):
            continue
        other = union(iv for q in queues if q != r["Queue_Id"] for iv in hv[q])
        tail_total += r["e"] - r["s"]
        tail_hidden += length(intersect([[r["s"], r["e"]]], other))
    sums = collections.defaultdict(float)
    for r in pipe:
        sums[short(r["Kernel_Name"]).split("<")[0]] += (r["e"] - r["s"]) / 1e6 / steps
    idle = (t1 - t0) - length(hv_all)
    return dict(trace=path, steps=steps, queues=queues, window_ms_per_step=round((t1 - t0) / 1e6 / steps, 4),
                no_throughput_kernel_resident_ms_per_step=round(idle / 1e6 / steps, 4),
                no_throughput_kernel_resident_share=round(idle / (t1 - t0), 4),
                throughput_overlap_between_lanes_share=round(length(union(both)) / max(1, length(hv_all)), 4),
                tail_under_other_lane_share=round(tail_hidden / max(1, tail_total), 4),
                throughput_kernels_ms_per_step=round(sum(v for k, v in sums.items() if k in THROUGHPUT), 4),
                kernel_ms_per_step={k: round(v, 4) for k, v in sorted(sums.items(), key=lambda kv: -kv[1])})


def one_step(path, k):
    rows = load(path)
    idx = [i for i, r in enumerate(rows) if "match_mfma" in r["Kernel_Name"]]
    k = len(idx) - 2 if k is None else k
    s = idx[k]
    e = next((i for i in idx if i > s + 1 and rows[i]["s"] > rows[s]["e"] + 2_000_000), len(rows))
    t0 = rows[s]["s"]
    for r in rows[s:min(e, s + 45)]:
        a, b = r["s"] - t0, r["e"] - t0
        print("%-40s q%s %8.1f %8.1f  %7.1f us" % (short(r["Kernel_Name"])[:40], r["Queue_Id"], a / 1e3, b / 1e3, (b - a) / 1e3))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summary":
        d = summary(sys.argv[3], int(sys.argv[2]))
        text = json.dumps(d, indent=1)
        if len(sys.argv) > 4:
            with open(sys.argv[4], "w") as f:
                f.write(text + "\n")
        print(text)
    else:
        one_step(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else None)
