#!/usr/bin/env python3
"""Timeline of the last pass in a rocprofv3 kernel trace of `python bench.py` (c3), and how much of every selection / sweep
launch of device batch b lies inside the distance GEMM of batch b + 1 (profiles/overlap_c3.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py
    python scripts/overlap_share.py DIR/NAME_kernel_trace.csv
"""
import csv
import re
import sys


def short(name):
    m = re.search(r'(k_\w+|__amd_rocclr_\w+)(<[^>]*>)?', name)
    return (m.group(1) + (m.group(2) or '')) if m else name[:40]


def main(path):
    rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name']), r['Stream_Id'])
            for r in csv.DictReader(open(path))]
    rows.sort()
    # a pass = the launches between two idle gaps of more than 0.5 ms (the host between two steps: the copy back, the next upload); the last one with three GEMM launches or more
    # (idle = none of the pass's own kernels running: the next step's upload and packing start inside the gap)
    passes, busy_until = [[]], 0
    for r in rows:
        main_kernel = re.match(r'k_(jc69|select|lean|sweep)', r[2]) is not None
        if main_kernel and passes[-1] and busy_until and r[0] - busy_until > 5e5:
            passes.append([])
        passes[-1].append(r)
        if main_kernel:
            busy_until = max(busy_until, r[1])
    last = [p for p in passes if sum(r[2].startswith('k_jc69_gemm') for r in p) >= 3][-1]
    while not last[0][2].startswith('k_jc69_gemm'):
        last.pop(0)  # (the first chunk's upload and packing)
    t0 = last[0][0]
    end = max(r[1] for r in last)
    print('last pass: %.3f ms from the first GEMM launch to the last kernel end' % ((end - t0) / 1e6))
    print('%10s %10s %9s  %-7s %s' % ('start ms', 'end ms', 'ms', 'stream', 'kernel'))
    g = [r for r in last if r[2].startswith('k_jc69_gemm')]
    for s, e, n, st in last:
        if e - s < 20000 and not n.startswith('k_jc69_gemm'):
            continue  # (memsets, packing: below 20 us)
        line = '%10.3f %10.3f %9.3f  %-7s %s' % ((s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6, st, n)
        if re.match(r'k_(lean|select|sweep_lean)', n):
            inside = sum(max(0, min(e, ge) - max(s, gs)) for gs, ge, _, _ in g)
            line += '   %.0f %% inside a GEMM' % (100.0 * inside / max(e - s, 1))
        print(line)
    busy = sum(e - s for s, e, n, _ in g)
    print('GEMM launches of the pass: %d, %.3f ms in all' % (len(g), busy / 1e6))


if __name__ == '__main__':
    main(sys.argv[1])
