"""Level-2 launches inside a kernel trace of the default bench command: duration, grid, CU-us, and how much of each launch's time
other lanes' kernels (other queues) were running too.  python tools/trace_level2.py DB"""
import sqlite3
import sys
from collections import defaultdict

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if "kernel_dispatch" in t][0]
ks = [t for t in tabs if "kernel_symbol" in t][0]
cols = [r[1] for r in cur.execute(f"pragma table_info({kd})")]
qcol = "queue_id" if "queue_id" in cols else None
rows = list(cur.execute(f"select s.kernel_name, d.start, d.end, d.grid_size_x, d.workgroup_size_x, {'d.' + qcol if qcol else '0'} "
                        f"from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"))
print("dispatches", len(rows), "queues", sorted({r[5] for r in rows}))
# timed part: the last 60 % of the trace (warm-up, capture and eager passes come first)
t_lo = rows[0][1] + 0.4 * (rows[-1][2] - rows[0][1])
rows = [r for r in rows if r[1] >= t_lo]
import bisect
starts = [r[1] for r in rows]
stats = defaultdict(list)
for i, (name, s, e, gx, wx, q) in enumerate(rows):
    if "window96_kernel" not in name:
        continue
    hid = "384" if "ILi384" in name else "192"
    # overlap: time in [s, e) covered by kernels of other queues
    lo = bisect.bisect_left(starts, s - 400_000)
    iv = []
    for n2, s2, e2, _, _, q2 in rows[lo:]:
        if s2 >= e:
            break
        if q2 != q and e2 > s:
            iv.append((max(s, s2), min(e, e2)))
    iv.sort()
    cov, cur_e = 0, s
    for a, b in iv:
        a = max(a, cur_e)
        if b > a:
            cov += b - a
            cur_e = b
    stats[(hid, gx // wx, wx)].append(((e - s) / 1e3, cov / (e - s), len(iv)))
for (hid, grid, wg), v in sorted(stats.items()):
    d = sorted(x[0] for x in v)
    print(f"window96 hid {hid} grid {grid} x {wg}: n {len(v)}  mean {sum(d) / len(d):.1f} us  median {d[len(d) // 2]:.1f}  min {d[0]:.1f}  max {d[-1]:.1f}  "
          f"workgroups x mean {grid * sum(d) / len(d):.0f}  time with another queue busy {sum(x[1] for x in v) / len(v):.2f}  "
          f"other-queue kernels overlapping {sum(x[2] for x in v) / len(v):.1f}")
