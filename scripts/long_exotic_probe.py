"""dist_ms of the fused JC69 pass at L = 10 000 where the reference rows hold N: (a) a clean reference, (b) N at 1 % of the sites of
1 per mille of the rows, (c) N at 1 % of the sites of every row -- each on the context's default route (the K-split GEMM, for (b) and
(c) its EX form with k_long_exotic_fix behind it: csrc/dist_gemm.hip, csrc/dist.hip) and, for (b) and (c), on the 8-plane
bit-plane kernel (no_dist_gemm: what such references ran on before).  200 000 leaves x 10 000 resident queries by default; the
alignments are config 3's 1 000 columns repeated (the N pattern with them).  One process, a warm-up pass per leg, then
alternating repeats.  dist_ms covers both kernels of the route; the fix kernel's own time wants a kernel trace of this script.

    python scripts/long_exotic_probe.py [n_leaves] [n_queries] [repeats] [legs, e.g. a,b,c,b8,c8]
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
want = sys.argv[4].split(',') if len(sys.argv) > 4 else ['a', 'b', 'c', 'b8', 'c8']
L = 10000
ds = synth.make_dataset(n_leaves, 1000, nq)
nodes = np.array([ds.tree.name_to_node[n] for n in ds.ref_names], np.int32)
rng = np.random.default_rng(5)
hit = rng.integers(0, 100, ds.ref_seqs.shape, dtype=np.uint8) == 0  # 1 % of the sites
some = np.zeros(n_leaves, bool)
some[rng.choice(n_leaves, max(1, n_leaves // 1000), replace=False)] = True
refs = {'a': ds.ref_seqs, 'b': np.where(hit & some[:, None], np.uint8(ord('N')), ds.ref_seqs), 'c': np.where(hit, np.uint8(ord('N')), ds.ref_seqs)}
qry = np.tile(ds.query_seqs, (1, L // 1000))
legs = []
for name in want:
    eng = Engine(ds.tree, np.tile(refs[name[0]], (1, L // 1000)), nodes, method='OLS', debug=('no_dist_gemm',) if name.endswith('8') else ())
    h, _ = eng.upload_queries(qry)
    eng.place_resident(h)  # warm-up
    legs.append((name, eng, h, []))
    info = eng.describe()
    print(name, '->', info['fused_distance_pass'], 'planes', info['code_planes'], 'max such sites per row', info['exotic_sites_max_per_row'],
          'fixes', info.get('k_split_exotic_fixes'), flush=True)
for r in range(reps):
    for name, eng, h, ms in legs:
        eng.place_resident(h)
        ms.append(eng.timing()['dist_ms'])
print('leaves %d  queries %d  sites %d  repeats %d' % (n_leaves, nq, L, reps))
med = {}
for name, eng, h, ms in legs:
    ms = np.array(ms)
    med[name] = np.median(ms)
    print('%-3s dist_ms median %9.2f  min %9.2f  max %9.2f' % (name, med[name], ms.min(), ms.max()), flush=True)
for x in 'bc':
    if x in med and 'a' in med:
        print('(%s) / (a): %.3f x' % (x, med[x] / med['a']))
    if x in med and x + '8' in med:
        print('(%s) 8-plane valu / k-split: %.2f x' % (x, med[x + '8'] / med[x]))
