"""Clustered JC69 references of 8 192 to 65 535 sites with bytes beyond ACGT- (N . ? * n) keep the long fused route by representatives
(csrc/dist_gemm.hip: k_jc69_gemm_long's EX form over the representatives' image, dist.hip: k_long_exotic_fix behind it; select.hip:
k_cluster_dist_mfma<LONG, EX> and the k term of the long by-query forms), byte for byte against the C oracle.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle_c import COracle  # noqa: E402

from apples_amd.engine import Engine  # noqa: E402
from test_gpu_clustered_exotic import ACGT, _inputs, _own_rows  # noqa: E402

pytestmark = pytest.mark.gpu
_want = {}


def _oracle(inputs, lut=None, own_rows=False, **kw):
    """The C oracle, once per case (no distance table beyond 8 192 sites; at 8 192 the engine's own)."""
    key = (inputs, own_rows, tuple(sorted(kw.items())))
    if key not in _want:
        tree, ref, qry, nodes, ca = _inputs(*inputs)
        kw = dict(kw)
        co = COracle(tree, ref, nodes, clusters=ca, method=kw.pop('method', 'OLS'), criterion=kw.pop('criterion', 'MLSE'), lut=lut,
                     threads=len(os.sched_getaffinity(0)), **kw)
        _want[key] = co.place_sequences(*(_own_rows(inputs) if own_rows else (qry,)))
    return _want[key]


def _check(inputs, debug=(), own_rows=False, then=(), **kw):
    """The context of `inputs` places their queries, then those of every entry of `then` (same rows, other queries): one engine, the
    route's reports at the end.  A block whose queries all hold such bytes runs on the 8-plane forms, so the K-split launches are
    those of the clean blocks behind it."""
    tree, ref, qry, nodes, ca = _inputs(*inputs)
    flagged = not np.isin(ref, ACGT).all()
    eng = Engine(tree, ref, nodes, clusters=ca, debug=debug, **{'method': 'OLS', **kw})
    assert (eng._lut is None) == (ref.shape[1] > 8192)
    got = [eng.place_sequences(*(_own_rows(i) if own_rows else (_inputs(*i)[2],))) for i in (inputs,) + tuple(then)]
    info, lut = eng.describe(), eng._lut
    eng.close()
    assert info['code_planes'] == 2 and info['cluster_fused'] == 1 and info['eight_plane_copy'] == 1, info
    assert (info['cluster_exotic_clusters'] > 0) == flagged and info['cluster_k_split_launches'] >= 1, info
    assert (info['cluster_k_split_exotic_fixes'] >= 1) == (flagged and inputs[2]), info  # (only flagged representatives need the pass)
    assert info['cluster_blocks'] > 0 or len(ref) < 1024 or 'no_blocks' in debug, info
    for i, g in zip((inputs,) + tuple(then), got):
        assert g.tobytes() == _oracle(i, lut, own_rows, **kw).tobytes(), i
    return _oracle(inputs, lut, own_rows, **kw)


@pytest.mark.parametrize('L,reps', [(8192, True), (8193, False), (8193, True), (3 * 3840 + 1, True), (65535, True)])
def test_placements_match_the_oracle(L, reps):
    """The caller's table (its last passing counts loosened); the first word group beyond the query's LDS copy, members only and
    consensus rows too; three splits and a ragged word; the top of the packed totals."""
    inputs = (L, 320 if L > 60000 else 600, reps)
    want = _check(inputs)
    assert want['n_obs'][7] == 0 and (want['n_obs'] > 64).any()  # (the all-gap query; a cluster of more than 64 members was accepted)
    if L == 8193:  # the recount matters: such bytes as gaps give other placements
        assert _oracle(inputs + (0, True)).tobytes() != want.tobytes()


@pytest.mark.parametrize('kw', [dict(threshold=0.02, baseobs=25), dict(overlap=0.52), dict(method='FM', criterion='HYBRID')], ids=str)
def test_rules_and_records(kw):
    """Phase 4 by query; valid / L about 0.525: the loosened screen around the overlap rule; the per-edge records."""
    _check((8193, 600, True), **kw)


@pytest.mark.parametrize('n,debug', [(600, ('no_cluster_mfma',)), (600, ('no_blocks',)), (1200, ()), (1200, ('no_cluster_mfma',)), (1200, ('no_blocks',))], ids=str)
def test_same_bytes_under_the_debug_switches_and_with_clade_blocks(n, debug):
    """The bit-count form with its k term; 1 200 leaves: the lean sweep and the clade blocks over flagged members, own rows and exact
    matches (an ex_block for the two flagged copies)."""
    want = _check((8193, n, True), debug=debug, own_rows=n == 1200)
    assert n == 600 or ((want['flags'][200:210] & 1).all() and not (want['flags'][100:192] & 1).any())  # F_EXACT


@pytest.mark.parametrize('first,then', [((8193, 600, True, 3), [(8193, 600, True)]), ((8193, 600, True, 100), [(8193, 600, True)]),
                                        ((8193, 600, True, 0, True), [(8193, 600, True, 3, 'ctx'), (8193, 600, True, 0, True)])], ids=str)
def test_query_blocks_with_such_bytes_keep_the_panels(first, then):
    """3 of 300 queries with such bytes (an ex_block), 100 (the whole block on the 8-plane forms), and a clean context that meets
    such a block: nothing is re-packed, the clean block behind it is fused again."""
    _check(first, then=then)
