"""Kernel statistics of a `rocprofv3 --kernel-trace --stats` run of `tools/nodeclf_probe.py --trace-only`, read from
the run's results database (rocprofv3 writes its trace there; the `kernels` view holds one row per dispatch): per
kernel the calls, total / mean / min / max time and share, as rocprofv3's kernel stats list them, then the library's
kernels per call in launch order.

  rocprofv3 --kernel-trace --stats -d OUT -o nodeclf -- python tools/nodeclf_probe.py --trace-only
  python tools/nodeclf_trace_stats.py OUT/nodeclf_results.db > profiles/nodeclf_kernel_trace.txt

usage: python tools/nodeclf_trace_stats.py RESULTS_DB
"""
import sqlite3, re, sys, collections
db = sys.argv[1]
c = sqlite3.connect(db)
rows = list(c.execute("select name, start, end from kernels order by start"))
def short(n):
    n = n.replace('(anonymous namespace)::', '').replace('void ', '')
    depth = 0; out = ''
    for ch in n:
        if ch == '<': depth += 1
        if ch == '>': depth -= 1
        if ch == '(' and depth == 0: break
        out += ch
    return out.strip()
names = [short(r[0]) for r in rows]
dur = [r[2] - r[1] for r in rows]
tot = sum(dur)
st = collections.OrderedDict()
for n, d in zip(names, dur):
    s = st.setdefault(n, [0, 0, 1e30, 0]); s[0] += 1; s[1] += d; s[2] = min(s[2], d); s[3] = max(s[3], d)
print("# rocprofv3 --kernel-trace --stats of `python tools/nodeclf_probe.py --trace-only` on one MI355X")
print("# (10 forwards and 10 training steps - forward + BCE + backward + Adam - at n_iters 0, then at n_iters 7;")
print("#  hidden_dim 64, 32 x 50 hits / 225 segments, index inputs); kernel stats over the whole run:")
print("%-60s %6s %12s %10s %10s %10s %6s" % ("Name", "Calls", "TotalUs", "AverageUs", "MinUs", "MaxUs", "Pct"))
for n, (k, s, lo, hi) in sorted(st.items(), key=lambda kv: -kv[1][1]):
    print("%-60s %6d %12.1f %10.2f %10.2f %10.2f %6.2f" % (n[:60], k, s / 1e3, s / k / 1e3, lo / 1e3, hi / 1e3, 100.0 * s / tot))
# per call: the library's kernels (k_*) between torch / runtime kernels, grouped into runs
print()
print("# the library's kernels between two torch kernels, in launch order: each distinct run once, with how often it occurs\n# (forward calls in a row form one run: 22 kernels per forward at n_iters 7 -\n#  k_input, then 7 x (k_edge, k_node_walkW, k_node_mlpW) with the output network in the last k_node_mlpW; at n_iters 0\n#  the forward is k_input alone, which scores the hits)")
runs, cur = [], []
for n in names:
    if n.startswith('k_') or n.startswith('gnn::'):
        cur.append(n)
    else:
        if cur: runs.append(tuple(cur)); cur = []
if cur: runs.append(tuple(cur))
seen = collections.OrderedDict()
for r in runs:
    seen[r] = seen.get(r, 0) + 1
for r, k in seen.items():
    print("%4d x %3d kernels: %s" % (k, len(r), " ".join(r)))
