#!/usr/bin/env python3
"""Config 3's clustered shape (200 000 leaves, L = 1 000) with bytes beyond ACGT- in the QUERIES, in the manner of
scripts/query_exotic_legs.py: what a pass costs when many queries hold `N` and the reference is clustered (the command line's
default).  Query legs: clean; 10 % of the queries holding one `N`; 50 % holding ten; all holding 1 % `N`; half holding 200.
Reference legs: clean; `N` at 1 per mille of the members' sites (the consensus rows stay clean: D = 0); the same with 16 / with
200 `N` written into every CONSENSUS row -- the representatives' screen is then loosened by D = min(that, the block's largest
per-query count): the large-D legs.  `--off` sets APPLES_NO_CLUSTER_QUERY_EXOTIC (the 8-plane route, in this build); `--no-mfma`
sets the debug switch no_cluster_mfma (the bit-count member forms alone), `--qx-bitcount` APPLES_CLUSTER_QX_BITCOUNT (the bit-count
form for the tiles that hold a flagged query only).
Per leg: the ms of every resident pass (host clock), the phases' mean HIP-event times, D, launches of k_cluster_rep_query_fix.

    python scripts/clustered_query_exotic_legs.py [--tree DIR] [--off] [--no-mfma] [--refs a,b] [--steps K] > one_process.json
    python scripts/clustered_query_exotic_legs.py --table LABEL=a.json,b.json LABEL2=c.json ...   # median (min .. max) over the files

--tree DIR: import apples_amd from DIR (another commit's build); run the builds in alternating processes and hand the files to --table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--off', action='store_true')
ap.add_argument('--no-mfma', action='store_true')
ap.add_argument('--qx-bitcount', action='store_true')
ap.add_argument('--refs', default='clean,n-1permille,cons-16,cons-200')
ap.add_argument('--leaves', type=int, default=200000)
ap.add_argument('--queries', type=int, default=10000)
ap.add_argument('--steps', type=int, default=7)
ap.add_argument('--one-pass', action='store_true', help='one untimed pass per leg (for a kernel trace)')
ap.add_argument('--table', nargs='+')
args = ap.parse_args()

if args.table:
    cols = {}
    for spec in args.table:
        label, files = spec.split('=')
        for f in files.split(','):
            for leg, r in json.load(open(f)).items():
                cols.setdefault(leg, {}).setdefault(label, []).extend(r['pass_ms'])
                cols[leg]['D'] = max(cols[leg].get('D') or 0, r.get('D') or 0)
    labels = [s.split('=')[0] for s in args.table]
    print('%-28s %4s  ' % ('leg (reference / queries)', 'D') + '  '.join('%-26s' % x for x in labels))
    for leg, c in cols.items():
        print('%-28s %4d  ' % (leg, c['D']) + '  '.join('%-26s' % ('%.2f (%.2f .. %.2f)' % (np.median(c[x]), min(c[x]), max(c[x])) if x in c else '-') for x in labels))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.tree))
from apples_amd import synth, treecluster  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402
from apples_amd.fasta import Alignment  # noqa: E402
from apples_amd.reference import ReducedReference  # noqa: E402

L, Q = 1000, args.queries
ds = synth.make_dataset(args.leaves, L, Q)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
groups = treecluster.grouped(ds.tree, 0.2 * 1.2)
rng = np.random.default_rng(31)
res = {}


def with_n(share, count):
    q = ds.query_seqs[:Q].copy()
    rows = np.nonzero(rng.random(Q) < share)[0] if share < 1 else np.arange(Q)
    for _ in range(count):
        q[rows, rng.integers(0, L, size=len(rows))] = ord('N')
    return q


QUERIES = {'clean': ds.query_seqs[:Q], 'n-10pct-x1': with_n(0.1, 1), 'n-50pct-x10': with_n(0.5, 10), 'n-all-1pct': with_n(1.0, L // 100),
           'n-50pct-x200': with_n(0.5, 200)}


def legs(name, ref, cons_n):
    cons, rep_row, moff, mrow = ReducedReference(Alignment(ds.ref_names, ref), False, groups).cluster_arrays()
    if cons_n:  # N into every consensus row: what loosens the representatives' screen
        cons = cons.copy()
        for _ in range(cons_n):
            cons[np.arange(len(cons)), rng.integers(0, L, size=len(cons))] = ord('N')
    kw = {'knobs': {'APPLES_NO_CLUSTER_QUERY_EXOTIC': 1}} if args.off else {}
    if args.qx_bitcount:  # the tiles that hold a flagged query to k_cluster_dist_qx, the others stay on the matrix cores
        kw['knobs'] = {'APPLES_CLUSTER_QX_BITCOUNT': 1}
    if args.no_mfma:
        kw['debug'] = ('no_cluster_mfma',)
    eng = Engine(ds.tree, ref, nodes, clusters=(cons, rep_row, moff, mrow), method='OLS', criterion='MLSE', threshold=0.2, baseobs=25, overlap=0.001, **kw)
    for key, q in QUERIES.items():
        h, n = eng.upload_queries(np.ascontiguousarray(q))
        eng.place_resident(h)  # warm-up
        ph = {'dist_ms': 0.0, 'select_ms': 0.0, 'sweep_ms': 0.0}
        ms = []
        for _ in range(0 if args.one_pass else args.steps):
            t0 = time.perf_counter()
            eng.place_resident(h)
            eng.fetch(h, n)
            ms.append((time.perf_counter() - t0) * 1e3)
            tm = eng.timing()
            for k in ph:
                ph[k] += tm[k] / args.steps
        eng.free_queries(h)
        info = eng.describe()
        res[name + '/' + key] = {'pass_ms': ms, **ph, 'D': info.get('cluster_query_exotic_loosened_by'),
                                 'fixes': info.get('cluster_query_exotic_fixes'), 'cluster_fused': info.get('cluster_fused')}
        print(name + '/' + key, json.dumps(res[name + '/' + key]), file=sys.stderr, flush=True)
    eng.close()


permille = ds.ref_seqs.copy()
permille[rng.random(permille.shape) < 0.001] = ord('N')
REFS = {'clean': (ds.ref_seqs, 0), 'n-1permille': (permille, 0), 'cons-16': (permille, 16), 'cons-200': (permille, 200)}
for name in args.refs.split(','):
    legs(name, *REFS[name])
print(json.dumps(res))
