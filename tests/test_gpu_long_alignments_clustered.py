"""Clustered references on alignments of 8 192 to 65 535 sites: the fused selection by representatives in its long form
(csrc/dist_gemm.hip: k_jc69_gemm_long over the representatives' image; csrc/select.hip: the LONG forms), byte for byte against
the C oracle (no distance table beyond 8 192 sites).  Clade blocks run on the lean sweep only, from 2 048 tree nodes up: the
1 200-leaf case.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle_c import COracle  # noqa: E402

from apples_amd import synth, treecluster  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402
from apples_amd.fasta import Alignment  # noqa: E402
from apples_amd.reference import ReducedReference  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _inputs(L, n=600):
    """tests/test_gpu_long_alignments.py's rows (gap patterns, the all-gap query, the exact copy) under TreeCluster groups with
    consensus representatives; the smallest group of at least six leaves is cut into singletons, pairs and triples."""
    d = synth.make_dataset(320 if L > 60000 else n, L, 300, seed_tree=11, seed_aln=12, seed_query=13)
    rng = np.random.default_rng(L)
    ref, qry = d.ref_seqs.copy(), d.query_seqs.copy()
    ref[rng.random(ref.shape) < 0.3] = ord('-')
    qry[:, : L // 2][rng.random((len(qry), L // 2)) < 0.5] = ord('-')
    qry[7], qry[8] = ord('-'), ref[3]
    nodes = np.array([d.tree.name_to_node[n] for n in d.ref_names], np.int32)
    groups = sorted(treecluster.grouped(d.tree, 0.24 if L > 60000 else 0.3), key=lambda g: len(g[1]))
    small = groups.pop(next(i for i, g in enumerate(groups) if len(g[1]) >= 6))[1]
    cuts = np.cumsum([0] + [1 + k % 3 for k in range(len(small))])
    groups += [('cut%d' % k, small[a:b]) for k, (a, b) in enumerate(zip(cuts, cuts[1:])) if a < len(small)]
    sizes = [len(g[1]) for g in groups]
    assert max(sizes) > 64 and sum(2 <= s <= 32 for s in sizes) >= 3 and sizes.count(1) >= 1, sorted(sizes)
    return d.tree, ref, qry, nodes, ReducedReference(Alignment(d.ref_names, ref), False, groups).cluster_arrays()


def _oracle(L, lut=None, method='OLS', criterion='MLSE', n=600, qry=None, self_rows=None, **kw):
    tree, ref, q, nodes, ca = _inputs(L, n)
    co = COracle(tree, ref, nodes, clusters=ca, method=method, criterion=criterion, lut=lut, threads=len(os.sched_getaffinity(0)), **kw)
    return co.place_sequences(q if qry is None else qry, self_rows)


def _place(L, launches=True, method='OLS', criterion='MLSE', debug=(), n=600, qry=None, self_rows=None, **kw):
    """One pass; the route is (launches=False: is not) taken, and clade blocks ran exactly where the tree is big enough for them."""
    tree, ref, q, nodes, ca = _inputs(L, n)
    eng = Engine(tree, ref, nodes, clusters=ca, method=method, criterion=criterion, debug=debug, **kw)
    got = eng.place_sequences(q if qry is None else qry, self_rows)
    info = eng.describe()
    eng.close()
    assert info['code_planes'] == 2 and (info['cluster_k_split_launches'] >= 1) == launches, info
    assert not launches or (info['cluster_fused'] == 1 and (info['cluster_blocks'] > 0 or 'no_blocks' in debug)), info
    assert (info['block_items_last_batch'] > 0) == (n >= 1024 and launches and 'no_blocks' not in debug), info
    return got, eng._lut


@pytest.mark.parametrize('L', [8192, 8193, 3 * 3840 + 1, 20000, 65535])
def test_clustered_long_route_matches_the_oracle(L):
    """The caller's table still present (64 word groups); the first group past the query's LDS copy; three splits and a ragged
    word; valid counts past 8 191 with the screen's table in LDS; the top of the range (the table gathered from global memory)."""
    got, lut = _place(L)
    assert (lut is None) == (L > 8192)
    want = _oracle(L, lut=lut)
    assert want['n_obs'][7] == 0 and (want['n_obs'] > 64).any()  # (the all-gap query; a cluster of more than 64 members was accepted)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('kw', [dict(threshold=0.02, baseobs=25), dict(overlap=0.52), dict(method='FM', criterion='HYBRID')], ids=str)
def test_rules_and_records_at_65_groups(kw):
    """-f 0.02 -b 25 (as tests/test_gpu_scale.py's top-up test): most queries take phase 4, by-query arithmetic over the
    representative panel; -V 0.52 with valid / L about 0.525: pairs on both sides of the overlap rule; FM/HYBRID: the per-edge
    records ride the same lists."""
    got, _ = _place(8193, **kw)
    want = _oracle(8193, **kw)
    if 'baseobs' in kw:  # more than half the queries observe clusters beyond what the threshold alone accepts
        assert (want['n_obs'] > _oracle(8193, threshold=0.02, baseobs=0)['n_obs']).sum() > len(want) // 2
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('debug', [('no_blocks',), ('no_cluster_mfma',), ('no_dist_gemm',)])
def test_same_bytes_under_the_debug_switches(debug):
    """Without clade blocks; member distances by bit counts (k_cluster_dist's long form); without the K-split pass the general
    route still stands."""
    got, _ = _place(8193, launches=debug != ('no_dist_gemm',), debug=debug)
    assert got.tobytes() == _oracle(8193).tobytes()


def test_clade_blocks_on_the_long_route():
    """1 200 leaves (2 399 nodes: the lean sweep, so the blocks run): k_blocks_up / k_blocks_down behind the long forms, phase 3 over
    emission indices, item_bad in both member-distance kernels -- 100 queries are reference rows placed without their own row
    (the block that holds it is not whole), ten more equal a reference row (an exact match inside a block)."""
    qry = _inputs(8193, 1200)[2].copy()
    self_rows = np.full(len(qry), -1, np.int32)
    qry[100:210] = _inputs(8193, 1200)[1][400:510]
    self_rows[100:200] = np.arange(400, 500)
    want = _oracle(8193, n=1200, qry=qry, self_rows=self_rows)
    assert (want['flags'][200:210] & 1).all() and not (want['flags'][100:200] & 1).any()  # F_EXACT
    for debug in ((), ('no_cluster_mfma',), ('no_blocks',)):
        assert _place(8193, debug=debug, n=1200, qry=qry, self_rows=self_rows)[0].tobytes() == want.tobytes(), debug
