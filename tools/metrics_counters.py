"""Counter evidence for DESIGN §4 "Segment metrics": k_metrics under rocprofv3, 10 updates of 25.6 M segments each
(tools/metrics_probe.py --profile-target), kernel times from --kernel-trace --stats, and the atomic and read requests
(TCC_EA0_ATOMIC_sum, TCC_EA0_RDREQ_sum) from a --pmc run of its own.  Prints section 4 of
profiles/metrics_probe.txt; the rocprofv3 output goes under $OUT (default /tmp/metrics_counters).

  rocprofv3 --kernel-trace --stats -d $OUT/trace_<kind> -o run -- python tools/metrics_probe.py --profile-target <kind>
  rocprofv3 --pmc TCC_EA0_ATOMIC_sum TCC_EA0_RDREQ_sum -d $OUT/pmc -o run -- python tools/metrics_probe.py \\
      --profile-target clustered

usage: python tools/metrics_counters.py
"""
import glob
import os
import sqlite3
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("OUT", "/tmp/metrics_counters")
N = 25600000


def rocprof(args, tag, kind):
    d = os.path.join(OUT, tag)
    cmd = ["rocprofv3"] + args + ["-d", d, "-o", "run", "--", sys.executable,
                                   os.path.join(REPO, "tools", "metrics_probe.py"), "--profile-target", kind]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    return glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]


def kernel_us(db):
    c = sqlite3.connect(db)
    names = {r[0]: r[1] for r in c.execute("select id, kernel_name from rocpd_info_kernel_symbol")}
    ts = [(e - s) / 1e3 for k, s, e in c.execute("select kernel_id, start, end from rocpd_kernel_dispatch")
          if "k_metrics" in names.get(k, "")]
    return sum(ts) / len(ts), len(ts)


def counters(db):
    c = sqlite3.connect(db)
    out = {}
    for name, value in c.execute("select counter_name, value from counters_collection where kernel_name like "
                                 "'%k_metrics%'"):
        out.setdefault(name, []).append(value)
    return {k: sorted(v)[len(v) // 2] for k, v in out.items()}


def main():
    t_cl, k = kernel_us(rocprof(["--kernel-trace", "--stats"], "trace_clustered", "clustered"))
    t_one, _ = kernel_us(rocprof(["--kernel-trace", "--stats"], "trace_onebin", "onebin"))
    pmc = counters(rocprof(["--pmc", "TCC_EA0_ATOMIC_sum", "TCC_EA0_RDREQ_sum"], "pmc", "clustered"))
    at = pmc["TCC_EA0_ATOMIC_sum"]
    print("\n4. counters (tools/metrics_counters.py: rocprofv3 --kernel-trace --stats, then --pmc in a run of its own;"
          " %d updates of %d segments each)" % (k, N))
    print("  k_metrics, clustered scores, 1024 bins/octave   mean %7.1f us per launch" % t_cl)
    print("  k_metrics, one score value (every add merged)   mean %7.1f us per launch" % t_one)
    print("  TCC_EA0_ATOMIC_sum, clustered                   %.0f per launch = %.2f per segment" % (at, at / N))
    print("  TCC_EA0_RDREQ_sum, clustered                    %.0f per launch" % pmc["TCC_EA0_RDREQ_sum"])
    print("  -> scattered 64-bit histogram adds at %.1f G per second" % (at / t_cl / 1e3))


if __name__ == "__main__":
    main()
