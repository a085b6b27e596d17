#!/usr/bin/env python3
"""Config 3's size with bytes beyond ACGT- in the QUERIES (beside scripts/shape_legs.py, whose plumbing it borrows): what a pass
costs when many queries hold `N`.  Legs: clean; 10 % of the queries holding one `N`; 50 % holding ten; all holding 1 % `N`.
`--cap` adds the sweep behind QUERY_EXOTIC_CAP (api.hip): a reference with runs of `.` at both ends of every row and half of the
queries holding k `N` over those runs, k rising -- the screen's D = min(most such bytes in a reference row, k) rises with it.
Per leg: ms per call (host buffer in, placements out: the streamed entry, which learns the flags after a first pass), ms per pass of
the resident block, the phases' HIP-event times (dist = GEMM + the fix kernel behind it), D, launches of the fix kernel.

    python scripts/query_exotic_legs.py [--tree DIR] [--cap] [--queries Q] > query_exotic.json

--tree DIR: import apples_amd from DIR (another commit's build) for the comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--cap', action='store_true')
ap.add_argument('--queries', type=int, default=0)
ap.add_argument('--steps', type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
sys.path.insert(0, os.path.abspath(args.tree))
from apples_amd import synth  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402

n_leaves, L, Q, protein, method, thr = bench.WORKLOADS['c3']
Q = args.queries or Q
ds = synth.make_dataset(n_leaves, L, Q)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
rng = np.random.default_rng(29)
res = {}


def measure(eng, key, q):
    q = np.ascontiguousarray(q)
    eng.place_sequences(q)  # warm-up (and the 8-plane copies, the screen)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.place_sequences(q)
    call_ms = (time.perf_counter() - t0) / args.steps * 1e3
    h, n = eng.upload_queries(q)
    eng.place_resident(h)
    ph = {'dist_ms': 0.0, 'select_ms': 0.0, 'sweep_ms': 0.0, 'total_ms': 0.0}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.place_resident(h)
        tm = eng.timing()
        for k in ph:
            ph[k] += tm[k] / args.steps
    eng.fetch(h, n)
    pass_ms = (time.perf_counter() - t0) / args.steps * 1e3
    eng.free_queries(h)
    info = eng.describe()
    res[key] = {'ms_per_call': call_ms, 'ms_per_pass': pass_ms, **ph, 'D': info.get('query_exotic_loosened_by'),
                'query_exotic_fixes': info.get('query_exotic_fixes'), 'overlap': info.get('overlap')}
    print(key, json.dumps(res[key]), file=sys.stderr, flush=True)


def with_n(share, count):
    q = ds.query_seqs[:Q].copy()
    rows = np.nonzero(rng.random(Q) < share)[0] if share < 1 else np.arange(Q)
    for _ in range(count):
        q[rows, rng.integers(0, L, size=len(rows))] = ord('N')
    return q


eng = Engine(ds.tree, ds.ref_seqs, nodes, method=method, criterion='MLSE', threshold=thr, baseobs=25, overlap=0.001)
measure(eng, 'clean', ds.query_seqs[:Q])
measure(eng, 'n-10pct-x1', with_n(0.1, 1))
measure(eng, 'n-50pct-x10', with_n(0.5, 10))
measure(eng, 'n-all-1pct', with_n(1.0, L // 100))
eng.close()
if args.cap:
    ref = ds.ref_seqs.copy()
    ends = rng.integers(0, L // 6, size=(n_leaves, 2))
    col = np.arange(L)
    ref[(col[None, :] < ends[:, :1]) | (col[None, :] >= L - ends[:, 1:])] = ord('.')
    eng = Engine(ds.tree, ref, nodes, method=method, criterion='MLSE', threshold=thr, baseobs=25, overlap=0.001,
                 knobs={'APPLES_QUERY_EXOTIC_CAP': 8191})
    measure(eng, 'dots-clean-queries', ds.query_seqs[:Q])
    for k in (1, 4, 16, 64, 160):
        q = ds.query_seqs[:Q].copy()
        q[::2, :(k + 1) // 2] = ord('N')
        if k > 1:
            q[::2, L - k // 2:] = ord('N')
        measure(eng, 'dots-half-x%d' % k, q)
    eng.close()
print(json.dumps(res))
