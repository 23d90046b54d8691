#!/usr/bin/env python3
"""Per-launch kernel times of a rocprofv3 rocpd database, split by where a launch stands inside its MPC step.

    python3 scripts/rocpd_by_iteration.py DB [--skip STEPS] [--delimiter k_mpc_prologue]

scripts/rocpd_stats.py averages a kernel over all its launches; a kernel launched once per SQP iteration (the sweeps' partners, the
node pass, the head of the step, k_step_tail) then shows one figure for iterations that do different work.  Here the launches
are cut into steps at every launch of the delimiter kernel (k_mpc_prologue opens each agx_ocp_mpc_step), and the n-th launch of a
kernel within its step is reported on its own: count, mean, min, max in microseconds.  The first --skip steps (warm-up) are
left out."""
import argparse
import collections
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument("db")
ap.add_argument("--skip", type=int, default=5)
ap.add_argument("--delimiter", default="k_mpc_prologue")
a = ap.parse_args()
cur = sqlite3.connect(a.db).cursor()
cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
name_col = "name" if "name" in cols else "kernel_name"
rows = cur.execute(f"select {name_col}, start, end from kernels order by start").fetchall()


def short(name):
    s = name.split("(")[0]
    for p in ("void ", "agx_g0::", "agx_g1::", "agx::"):
        s = s.replace(p, "")
    return s


steps, cur_step = [], None
for name, s, e in rows:
    k = short(name)
    if k.startswith(a.delimiter):
        cur_step = collections.defaultdict(list)
        steps.append(cur_step)
    if cur_step is not None:
        cur_step[k].append((e - s) / 1e3)
steps = steps[a.skip:]
per = collections.defaultdict(list)  # (kernel, n-th launch within the step) -> durations
launches = collections.Counter()
for st in steps:
    launches[tuple(sorted((k, len(v)) for k, v in st.items()))] += 1
    for k, v in st.items():
        for n, d in enumerate(v):
            per[(k, n)].append(d)
print(f"{len(steps)} steps after {a.skip} skipped; {len(launches)} distinct launch pattern(s), the most common in {launches.most_common(1)[0][1]} steps")
print(f"{'kernel':48s} {'n-th':>4s} {'count':>6s} {'mean_us':>9s} {'min_us':>9s} {'max_us':>9s}")
total = 0.0
for (k, n), v in sorted(per.items(), key=lambda kv: (-sum(per[(kv[0][0], 0)]), kv[0][0], kv[0][1])):
    print(f"{k[:48]:48s} {n:4d} {len(v):6d} {sum(v) / len(v):9.2f} {min(v):9.2f} {max(v):9.2f}")
    total += sum(v)
print(f"all kernels of a step: {total / max(len(steps), 1):.1f} us")
