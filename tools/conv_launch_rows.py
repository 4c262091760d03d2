#!/usr/bin/env python3
"""Every conv_* launch of a whole rocprofv3 kernel trace by (kernel, workgroups): launches.
usage: conv_launch_rows.py <kernel_trace.csv> [prefix,prefix,...]   (default prefix: conv_; the float32 weight gradient's launches:
conv_wgrad_,wgrad_reduce_,pixel_table_kernel)"""
import collections
import csv
import sys

prefixes = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("conv_",)
g = collections.Counter()
for r in csv.DictReader(open(sys.argv[1])):
    n = r['Kernel_Name'].split('(')[0].replace('void ', '')
    if n.startswith(prefixes):
        g[(n, int(r['Grid_Size_X']) * int(r['Grid_Size_Y']) * int(r['Grid_Size_Z']) // int(r['Workgroup_Size_X']))] += 1
for (n, w), c in sorted(g.items()):
    print("%-60s %9d %6d" % (n, w, c))
