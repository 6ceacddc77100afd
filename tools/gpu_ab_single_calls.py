"""Same-box A/B of library builds on a timing tool's single-call rows, by the rule of profiles/ncc_single_as_batch.txt and profiles/ransac_single_as_batch.txt:
fresh processes of the tool, alternating parent, head, parent, head, ... (MULLS_HIP_LIB selects the build), every row the tool prints as
"... median [of N:] X ms (min Y, max Z)" collected per process.  A row passes if the median of head's process medians is at or below the median of the
parent's process medians plus the parent's spread (highest minus lowest of the parent's process medians).  Further builds named after head are run in the
same alternation and reported without a verdict.

    python tools/gpu_ab_single_calls.py --rounds 5 --libs parent=tools/_bin/libmulls_parent.so,head=mulls_amd/libmulls_hip.so -- python tools/gpu_ransac.py
"""
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = re.compile(r"^(.*?)\s+status .*?median(?: of +\d+:)? +([\d.]+) ms +\(min ([\d.]+), max ([\d.]+)\)")


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d  # noqa: E731
    rounds, libs, cmd = arg("--rounds", 5), [kv.split("=") for kv in arg("--libs", "").split(",")], sys.argv[sys.argv.index("--") + 1:]
    assert len(libs) >= 2 and libs[0][0] == "parent" and libs[1][0] == "head", "--libs parent=...,head=...[,name=...]"
    rows, seen = [], {name: {} for name, _ in libs}
    for r in range(rounds):
        for name, path in libs:
            env = dict(os.environ, MULLS_HIP_LIB=os.path.join(ROOT, path))
            p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:  # nothing more is started after a failure
                raise SystemExit("round %d, %s: exit %d\n%s\n%s" % (r, name, p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
            for line in p.stdout.split("\n"):
                m = ROW.match(line)
                if m:
                    key = re.sub(r"\s+", " ", m.group(1))
                    if key not in rows:
                        rows.append(key)
                    seen[name].setdefault(key, []).append(tuple(float(v) for v in m.group(2, 3, 4)))
            print("round %d %s done" % (r, name), file=sys.stderr, flush=True)
    print("per process: median (min, max) of its calls, ms\n")
    width = max(len(name) for name, _ in libs)
    for key in rows:
        print(key)
        for name, _ in libs:
            print("  %-*s %s" % (width, name, "  ".join("%.3f (%.3f, %.3f)" % t for t in seen[name][key])))
    print("\nsummary")
    others = [name for name, _ in libs[2:]]
    print("%-78s %13s %13s %11s %10s  %s%s" % ("row", "parent median", "parent spread", "head median", "bound", "verdict", "".join("  %s median" % o for o in others)))
    failed = 0
    for key in rows:
        pm, hm = [t[0] for t in seen["parent"][key]], [t[0] for t in seen["head"][key]]
        p, h, spread = statistics.median(pm), statistics.median(hm), max(pm) - min(pm)
        ok = h <= p + spread
        failed += not ok
        print("%-78s %13.3f %13.3f %11.3f %10.3f  %s (head / parent %.3f)%s"
              % (key, p, spread, h, p + spread, "pass" if ok else "FAIL", h / p, "".join("  %.3f" % statistics.median(t[0] for t in seen[o][key]) for o in others)))
    print("\n%d of %d rows fail" % (failed, len(rows)))


if __name__ == "__main__":
    main()
