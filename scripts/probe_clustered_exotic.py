"""Config 3's clustered shape (200 000 leaves, L = 1 000, 100 000 resident queries) three ways: clean; `N` at 1 per mille of the
reference sites; the same plus 1 % of the queries carrying an `N`.  The legs alternate (A B C A B C ...): every visit builds the
context, uploads the queries, warms up once and times resident passes with a host clock around place_resident (which ends in a
device synchronise): `--passes` of them, fewer once `--seconds` are full (the 8-plane route of a commit without the feature takes
twenty times as long per pass).  Prints per leg the visits' medians, so that the spread between visits of one leg stands beside the
differences between legs, and the route describe() reports.  Two commits are compared by running this file from a checkout of each
in turn, several times, in one session; `--legs 2` alone under a kernel trace gives the kernels' shares.

    python scripts/probe_clustered_exotic.py [--leaves N --queries Q --rounds R --passes P --seconds S --legs 0,1,2]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from apples_amd import synth, treecluster  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402
from apples_amd.fasta import Alignment  # noqa: E402
from apples_amd.reference import ReducedReference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leaves', type=int, default=200000)
    ap.add_argument('--length', type=int, default=1000)
    ap.add_argument('--queries', type=int, default=100000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--passes', type=int, default=60)
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--legs', default='0,1,2')
    args = ap.parse_args()
    ds = synth.make_dataset(args.leaves, args.length, args.queries)
    nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
    groups = treecluster.grouped(ds.tree, 0.2 * 1.2)
    rng = np.random.default_rng(1)
    ref_n = ds.ref_seqs.copy()
    ref_n[rng.random(ref_n.shape) < 0.001] = ord('N')
    qry_n = ds.query_seqs.copy()
    qry_n[rng.random(len(qry_n)) < 0.01, args.length // 2] = ord('N')
    legs = {'clean': (ds.ref_seqs, ds.query_seqs), 'N in the reference': (ref_n, ds.query_seqs), 'N in reference and queries': (ref_n, qry_n)}
    legs = {k: v for i, (k, v) in enumerate(legs.items()) if str(i) in args.legs.split(',')}
    arrays = {id(ref): ReducedReference(Alignment(ds.ref_names, ref), False, groups).cluster_arrays() for ref, _ in legs.values()}
    ms = {k: [] for k in legs}
    info = {}
    for _ in range(args.rounds):
        for name, (ref, qry) in legs.items():
            eng = Engine(ds.tree, ref, nodes, clusters=arrays[id(ref)], method='OLS', criterion='MLSE', threshold=0.2, baseobs=25, overlap=0.001)
            h, _ = eng.upload_queries(qry)
            eng.place_resident(h)
            t = []
            while len(t) < args.passes and (len(t) < 3 or sum(t) < args.seconds * 1e3):
                t0 = time.perf_counter()
                eng.place_resident(h)
                t.append((time.perf_counter() - t0) * 1e3)
            ms[name].append(statistics.median(t))
            info[name] = {'passes': len(t)}
            d = eng.describe()
            info[name].update({k: d[k] for k in ('code_planes', 'cluster_fused', 'eight_plane_copy', 'cluster_exotic_clusters', 'exotic_sites_max_per_row',
                                            'cluster_blocks') if k in d})
            info[name].update({k: round(float(v), 2) for k, v in eng.timing().items() if k.endswith('_ms')})
            eng.free_queries(h)
            eng.close()
    print('%d leaves, L = %d, %d resident queries; ms per pass, a visit = the median of up to %d passes (%g s)' % (args.leaves, args.length, args.queries, args.passes, args.seconds))
    for name in legs:
        print('%-28s visits %s  -> %.2f ms (spread %.2f)  %s' % (name, ' '.join('%.2f' % v for v in ms[name]), statistics.median(ms[name]),
                                                              max(ms[name]) - min(ms[name]), info[name]))


if __name__ == '__main__':
    main()
