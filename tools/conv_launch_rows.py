#!/usr/bin/env python3
"""Every conv_* launch of a whole rocprofv3 kernel trace by (kernel, workgroups): launches.  usage: conv_launch_rows.py <kernel_trace.csv>"""
import collections
import csv
import sys

g = collections.Counter()
for r in csv.DictReader(open(sys.argv[1])):
    n = r['Kernel_Name'].split('(')[0].replace('void ', '')
    if n.startswith('conv_'):
        g[(n, int(r['Grid_Size_X']) * int(r['Grid_Size_Y']) * int(r['Grid_Size_Z']) // int(r['Workgroup_Size_X']))] += 1
for (n, w), c in sorted(g.items()):
    print("%-60s %9d %6d" % (n, w, c))
