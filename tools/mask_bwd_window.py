#!/usr/bin/env python3
"""Mask-head backward window of one step: from the start of the mask output stage's backward (mask_out_bwd*) to the end of the
last ROIAlign adjoint (roialign_kernel<true>); per queue: launches and summed kernel time inside it; the Winograd transform rows."""
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
step = int(sys.argv[2]) if len(sys.argv) > 2 else 6
ev = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].split('(')[0].replace('void ', ''),
             int(r['Grid_Size_X']) * int(r['Grid_Size_Y']) * int(r['Grid_Size_Z']) // int(r['Workgroup_Size_X']), r['Queue_Id']) for r in rows)
sgd = [e for e in ev if e[2].startswith('sgd_kernel')]
t0, t1 = sgd[step][1], sgd[step + 1][1]
seg = [e for e in ev if e[0] >= t0 and e[1] <= t1]
a = next(e for e in seg if e[2].startswith('mask_out_bwd'))
b = [e for e in seg if e[2].startswith('roialign_kernel<true>')][-1]
w0, w1 = a[0], b[1]
win = [e for e in seg if e[0] >= w0 and e[1] <= w1]
print("step wall %.3f ms, %d launches; mask-head backward window %.3f ms (+%.3f .. +%.3f), %d launches" % (
    (t1 - t0) / 1e6, len(seg), (w1 - w0) / 1e6, (w0 - t0) / 1e6, (w1 - t0) / 1e6, len(win)))
for q in sorted(set(e[4] for e in win)):
    qs = [e for e in win if e[4] == q]
    print("queue %s: %d launches, summed kernel time %.3f ms" % (q, len(qs), sum(e[1] - e[0] for e in qs) / 1e6))
g = collections.defaultdict(lambda: [0, 0])
for e in win:
    if e[2].startswith('winograd_'):
        g[(e[4], e[2], e[3])][0] += 1; g[(e[4], e[2], e[3])][1] += e[1] - e[0]
print("Winograd launches in the window:")
for k, (c, t) in sorted(g.items(), key=lambda kv: -kv[1][1]):
    print("  q%s %-44s wgs=%6d n=%4d sum=%7.3f ms mean=%6.1f us" % (k[0], k[1][:44], k[2], c, t / 1e6, t / c / 1e3))
