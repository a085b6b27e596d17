"""Resident pass time of a CLUSTERED reference on a long alignment whose rows hold `N`: scripts/long_clustered_probe.py's shape
(config 3's tree of 200 000 leaves under TreeCluster groups with consensus representatives, its 1 000 columns repeated to
L = 10 000, 10 000 queries) with `N` at 1 % of the sites of about a third of the reference rows and, likewise, of the consensus rows
(a majority consensus of such rows holds none by itself; real ones do where most members have one).  Legs, alternating in one process
after a warm-up pass each:

    a  the long fused route with the mask planes (k_jc69_gemm_long's EX form + k_long_exotic_fix over the representatives,
       k_cluster_dist_mfma<LONG, EX> for the flagged clusters' tiles)
    b  the same inputs under no_dist_gemm: 8 planes, no panels, full rows and the general selection -- the route these inputs took
       before the long forms knew the mask planes (a checkout of such a commit runs leg a on that route: same script, both sides)
    c  the clean reference on the long fused route
    d  leg a with no_cluster_mfma: the member distances by bit counts (k_cluster_dist<LONG> with its k term)

Legs a, b and d must place every query alike (checked).  A kernel trace of leg a alone (`... a`) gives the kernels' shares.

    python scripts/long_clustered_exotic_probe.py [n_leaves] [n_queries] [repeats] [legs]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from apples_amd import synth, treecluster  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402
from apples_amd.fasta import Alignment  # noqa: E402
from apples_amd.reference import ReducedReference  # noqa: E402

n_leaves = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
which = sys.argv[4] if len(sys.argv) > 4 else 'abcd'
K = 10  # L = 10 000
ds = synth.make_dataset(n_leaves, 1000, nq)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
groups = treecluster.grouped(ds.tree, 0.2 * 1.2)
rng = np.random.default_rng(1)
ref_n = ds.ref_seqs.copy()
ref_n[(rng.random(len(ref_n)) < 1 / 3)[:, None] & (rng.random(ref_n.shape) < 0.01)] = ord('N')
KEYS = ('fused_distance_pass', 'cluster_fused', 'cluster_blocks', 'code_planes', 'eight_plane_copy', 'cluster_exotic_clusters',
        'exotic_sites_max_per_row', 'n_reps')
legs = []
for name, ref, debug in (('a N, fused', ref_n, ()), ('b N, no_dist_gemm', ref_n, ('no_dist_gemm',)), ('c clean, fused', ds.ref_seqs, ()),
                         ('d N, no_cluster_mfma', ref_n, ('no_cluster_mfma',))):
    if name[0] not in which:
        continue
    # (the consensus of repeated columns is the repeated consensus; consensus rows follow the reference rows, same indices)
    cons, rep_row, member_off, member_row = ReducedReference(Alignment(ds.ref_names, ref), False, groups).cluster_arrays()
    cons = np.asarray(cons, np.uint8).reshape(-1, 1000).copy()
    if ref is ref_n:
        cons[(np.random.default_rng(2).random(len(cons)) < 1 / 3)[:, None] & (np.random.default_rng(3).random(cons.shape) < 0.01)] = ord('N')
    ca = (np.tile(cons, (1, K)), rep_row, member_off, member_row)
    eng = Engine(ds.tree, np.tile(ref, (1, K)), nodes, clusters=ca, method='OLS', debug=debug)
    h, _ = eng.upload_queries(np.tile(ds.query_seqs, (1, K)))
    eng.place_resident(h)  # warm-up
    legs.append((name, eng, h, [], eng.fetch(h, nq).tobytes()))
    info = eng.describe()
    print(name, '->', {x: info.get(x) for x in KEYS}, flush=True)
same = {l[0]: l[4] == legs[0][4] for l in legs if ' N' in l[0]}
print('placements of the legs with N equal to the first such leg:', same, flush=True)
for r in range(reps):
    for name, eng, h, rows, _ in legs:
        eng.place_resident(h)
        t = eng.timing()
        rows.append([t['total_ms'], t['dist_ms'], t['select_ms'], t['blocks_ms'], t['sweep_ms']])
print('leaves %d  queries %d  repeats %d  clusters %d  L %d' % (n_leaves, nq, reps, info['n_reps'], 1000 * K))
med = {}
for name, eng, h, rows, _ in legs:
    a = np.array(rows)
    med[name[0]] = np.median(a[:, 0])
    d = eng.describe()
    print('%-22s total_ms median %8.2f  min %8.2f  max %8.2f | representatives %7.2f  selection + members %7.2f  blocks %6.2f  sweep %7.2f'
          ' | k-split launches %s  fixes %s' % ((name, med[name[0]], a[:, 0].min(), a[:, 0].max()) + tuple(np.median(a[:, 1:], axis=0)) +
                                                (d.get('cluster_k_split_launches'), d.get('cluster_k_split_exotic_fixes'))))
for x, y, what in (('b', 'a', '8-plane general route / fused route with N'), ('a', 'c', 'fused route with N / clean'),
                   ('d', 'a', 'bit-count member distances / matrix-core ones, with N')):
    if x in med and y in med:
        print('%s: %.2f x' % (what, med[x] / med[y]))
if not all(same.values()):
    sys.exit('the legs with N disagree')
