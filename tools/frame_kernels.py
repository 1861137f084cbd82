"""Per-frame kernel times of a blocking-frame run under rocprofv3 --kernel-trace: python tools/frame_kernels.py <output dir> [frames] [start kernel]

A frame starts at a k_raygen (or k_ingest, or k_ingest_hits) dispatch; with `start kernel` only the frames that start with that kernel count (a run
that makes passes of two kinds, tools/shade_hits_bench.py).  The last `frames` frames (default 5) are averaged; every kernel is named with its position
among the frame's launches of that kernel (k_shade #0, #1, ...) and, in brackets, the instantiation that ran.  The layout of profiles/shade_finish."""
import collections, csv, glob, re, sys

d = sys.argv[1]
keep = int(sys.argv[2]) if len(sys.argv) > 2 else 5
only = sys.argv[3] if len(sys.argv) > 3 else None
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[-1]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
rows = [r for r in rows if "xrt::" in r["Kernel_Name"]]
frames, cur = [], None
for r in rows:
    full = re.sub(r"^void ", "", r["Kernel_Name"]).replace("xrt::", "")
    inst = re.match(r"[\w]+(<[^(]*>)?", full).group(0)
    short = re.match(r"\w+", inst).group(0)
    if short in ("k_raygen", "k_ingest", "k_ingest_hits"):
        cur = []
        frames.append(cur)
    if cur is not None:
        cur.append((short, inst, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
frames = [fr for fr in frames if only is None or fr[0][0] == only]
frames = [fr for fr in frames if len(fr) == len(frames[-1])][-keep:]
print("frames averaged: %d; frame (first start to last end) us: %s" % (len(frames), " ".join("%.1f" % ((max(k[3] for k in fr) - fr[0][2]) / 1e3) for fr in frames)))
table, order, sums = collections.defaultdict(list), [], collections.defaultdict(lambda: [0.0] * len(frames))
for i, fr in enumerate(frames):
    seen = collections.Counter()
    for short, inst, s, e in fr:
        key = (short, seen[short], inst)
        seen[short] += 1
        if key not in table:
            order.append(key)
        table[key].append((e - s) / 1e3)
        sums[short][i] += (e - s) / 1e3
for key in order:
    v = table[key]
    print("%-16s #%d  mean %9.1f us   per frame: %s   [%s]" % (key[0], key[1], sum(v) / len(v), " ".join("%.1f" % x for x in v), key[2]))
for short, v in sums.items():
    print("SUM %-16s mean %9.1f us   per frame: %s" % (short, sum(v) / len(v), " ".join("%.1f" % x for x in v)))
