"""dist_ms of the fused JC69 pass on long alignments: the K-split GEMM (csrc/dist_gemm.hip: k_jc69_gemm_long) at L = 10 000, the same
context on the bit-plane kernel (no_dist_gemm: what such alignments ran on before), and k_jc69_gemm's 2^12 form at L = 4 000.
200 000 leaves x 10 000 queries by default; the alignments are config 3's 1 000 columns repeated, so all legs see the same
distances and survivors.  One process, a warm-up pass per leg, then alternating repeats.

    python scripts/long_alignment_probe.py [n_leaves] [n_queries] [repeats]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from apples_amd import synth  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402

n_leaves = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ds = synth.make_dataset(n_leaves, 1000, nq)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
legs = []
for name, L, debug in (('k-split gemm L=10000', 10000, ()), ('bit-plane valu L=10000', 10000, ('no_dist_gemm',)),
                       ('gemm 2^12 L=4000', 4000, ())):
    eng = Engine(ds.tree, np.tile(ds.ref_seqs, (1, L // 1000)), nodes, method='OLS', debug=debug)
    h, _ = eng.upload_queries(np.tile(ds.query_seqs, (1, L // 1000)))
    eng.place_resident(h)  # warm-up
    legs.append((name, L, eng, h, []))
    print(name, '->', eng.describe()['fused_distance_pass'], flush=True)
for r in range(reps):
    for name, L, eng, h, ms in legs:
        eng.place_resident(h)
        ms.append(eng.timing()['dist_ms'])
print('leaves %d  queries %d  repeats %d  packed_bytes(L=10000) %d' % (n_leaves, nq, reps, legs[0][2].describe()['packed_bytes']))
per = {}
for name, L, eng, h, ms in legs:
    ms = np.array(ms)
    per[name] = np.median(ms) / (float(nq) * n_leaves * L) * 1e12
    print('%-24s dist_ms median %9.2f  min %9.2f  max %9.2f   fs per query x leaf x site %.3f' % (name, np.median(ms), ms.min(), ms.max(), per[name] * 1e3))
names = [l[0] for l in legs]
print('valu / k-split at L=10000: %.2f x' % (per[names[1]] / per[names[0]]))
print('k-split per site against the L=4000 gemm: %.3f x' % (per[names[0]] / per[names[2]]))
