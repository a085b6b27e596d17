"""Resident pass time of a CLUSTERED reference on a long alignment: config 3's tree (200 000 leaves) under TreeCluster groups at the
default 1.2 x f with consensus representatives, L = 10 000, 10 000 queries -- the fused selection by representatives in its long
form (csrc/dist_gemm.hip: k_jc69_gemm_long over the representatives' image; csrc/select.hip: the LONG forms), with the split of
the pass: representatives' pass (dist_ms), selection + member distances (select_ms), clade blocks (blocks_ms), sweep (sweep_ms).
A second leg is the same reference at L = 1 000 (`c3-clustered`), for the cost per site.  The alignments are config 3's 1 000
columns repeated, so both legs see the same distances, clusters and survivors.  On a commit without the route the L = 10 000
leg falls back to full rows and the general selection: the same script measures both sides; the third leg (no_dist_gemm: no
panels beyond 8 192 sites) is that fall-back inside this process, for an alternating comparison.  One process, a warm-up pass per leg,
then alternating repeats.

    python scripts/long_clustered_probe.py [n_leaves] [n_queries] [repeats]
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
ds = synth.make_dataset(n_leaves, 1000, nq)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
cons, rep_row, member_off, member_row = ReducedReference(Alignment(ds.ref_names, ds.ref_seqs), False,
                                                         treecluster.grouped(ds.tree, 0.2 * 1.2)).cluster_arrays()
KEYS = ('fused_distance_pass', 'cluster_fused', 'cluster_blocks', 'cluster_k_split_launches', 'code_planes', 'n_reps', 'batch')
legs = []
for name, L, debug in (('clustered L=10000', 10000, ()), ('clustered L=1000', 1000, ()),
                       ('L=10000, no_dist_gemm', 10000, ('no_dist_gemm',))):
    k = L // 1000
    # (the consensus of repeated columns is the repeated consensus; consensus rows follow the reference rows, same indices)
    ca = (np.tile(np.asarray(cons, np.uint8).reshape(-1, 1000), (1, k)), rep_row, member_off, member_row)
    eng = Engine(ds.tree, np.tile(ds.ref_seqs, (1, k)), nodes, clusters=ca, method='OLS', debug=debug)
    h, _ = eng.upload_queries(np.tile(ds.query_seqs, (1, k)))
    eng.place_resident(h)  # warm-up
    legs.append((name, L, eng, h, []))
    info = eng.describe()
    print(name, '->', {x: info.get(x) for x in KEYS}, flush=True)
for r in range(reps):
    for name, L, eng, h, rows in legs:
        eng.place_resident(h)
        t = eng.timing()
        rows.append([t['total_ms'], t['dist_ms'], t['select_ms'], t['blocks_ms'], t['sweep_ms']])
print('leaves %d  queries %d  repeats %d  clusters %d' % (n_leaves, nq, reps, len(rep_row)))
med = {}
for name, L, eng, h, rows in legs:
    a = np.array(rows)
    med[name] = np.median(a[:, 0])
    print('%-18s total_ms median %8.2f  min %8.2f  max %8.2f | representatives %7.2f  selection + members %7.2f  blocks %6.2f  sweep %7.2f'
          % ((name, med[name], a[:, 0].min(), a[:, 0].max()) + tuple(np.median(a[:, 1:], axis=0))))
    print('   launches after the passes:', eng.describe().get('cluster_k_split_launches'))
names = [l[0] for l in legs]
print('pass time per site, L=10000 against L=1000: %.3f x' % ((med[names[0]] / 10000) / (med[names[1]] / 1000)))
print('fall-back / fused route at L=10000: %.2f x' % (med[names[2]] / med[names[0]]))
