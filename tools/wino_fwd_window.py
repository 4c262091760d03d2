#!/usr/bin/env python3
"""The Winograd transform launches of the mask-head FORWARD of one training step of a rocprofv3 kernel trace: the window from the
ProposalLayer to the transposed convolution's GEMM (winograd_gemm_kernel<.., true, ..>), where no backward launch of the same kernels
runs; grouped by (kernel, workgroups): launches, summed and mean duration.
usage: wino_fwd_window.py <kernel_trace.csv> [step index]"""
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
step = int(sys.argv[2]) if len(sys.argv) > 2 else 6
ev = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].split('(')[0].replace('void ', ''),
             int(r['Grid_Size_X']) * int(r['Grid_Size_Y']) * int(r['Grid_Size_Z']) // int(r['Workgroup_Size_X'])) for r in rows)
sgd = [e for e in ev if e[2].startswith('sgd_kernel')]
t0, t1 = sgd[step][1], sgd[step + 1][1]
seg = [e for e in ev if e[0] >= t0 and e[1] <= t1]
p = next(e for e in seg if e[2].startswith('select_sort_decode') or e[2].startswith('topk'))
d = next(e for e in seg if e[2].startswith(('winograd_gemm_kernel<2, true', 'winograd_gemm_kernel<4, true')))   # DECONV, with or without the mask epilogue
win = [e for e in seg if e[0] >= p[1] and e[1] <= d[0]]
print("mask-head forward window (ProposalLayer .. transposed convolution): %.3f ms" % ((d[0] - p[1]) / 1e6))
names = ('winograd_input_kernel', 'winograd_output_kernel', 'winograd_chain_kernel')
g = collections.defaultdict(lambda: [0, 0])
for s, e, n, wgs in win:
    if n.startswith(names):
        g[(n, wgs)][0] += 1; g[(n, wgs)][1] += e - s
print("%-40s %9s %4s %9s %9s" % ("kernel", "workgroups", "n", "sum ms", "mean us"))
for (n, wgs), (c, t) in sorted(g.items()):
    print("%-40s %9d %4d %9.3f %9.1f" % (n, wgs, c, t / 1e6, t / c / 1e3))
print("%-40s %9s %4d %9.3f" % ("all transform launches of the window", "", sum(c for c, _ in g.values()), sum(t for _, t in g.values()) / 1e6))
