"""Clustered JC69 query blocks in which many queries hold bytes beyond ACGT- (N . ? * n R y) stay on the fused route by
representatives (csrc/select.hip: k_cluster_rep_query_fix, the QX forms of the member-distance kernels), byte for byte against the
C oracle.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle_c import COracle  # noqa: E402

from apples_amd import synth, treecluster  # noqa: E402
from apples_amd.engine import Engine, jc69_lut  # noqa: E402
from apples_amd.fasta import Alignment  # noqa: E402
from apples_amd.reference import ReducedReference  # noqa: E402

pytestmark = pytest.mark.gpu
EX, ACGT = np.frombuffer(b'N.?*nRy', np.uint8), np.frombuffer(b'ACGT-', np.uint8)


def _sprinkle(rows, rng, frac=1.0, keep=(), rate=0.01):
    """Such bytes at about `rate` of the sites of about `frac` of the rows (never in the rows `keep`)."""
    at = (rng.random(len(rows)) < frac)[:, None] & (rng.random(rows.shape) < rate)
    at[list(keep)] = False
    rows[at] = rng.choice(EX, int(at.sum()))


@functools.lru_cache(maxsize=None)
def _inputs(L=1001, n=600, flagged=True, edge=False, own=False):
    """tests/test_gpu_clustered_exotic.py's rows and groups (600 leaves, 300 queries, 30 % gaps, the cut-up small cluster).  Queries
    10..109 hold such bytes at 1 % of their sites; 20..39 are near copies of row r of the biggest cluster.  flagged: members and
    consensus rows hold such bytes too, r and its consensus row N at shared sites, which 20..29 copy and 30..39 hold as n.  edge: an
    all-N query and one whose only such byte is a ? in the last, ragged word.  own: 150..249 are reference rows, eight of them flagged."""
    d = synth.make_dataset(n, L, 300, seed_tree=11, seed_aln=12, seed_query=13)
    rng = np.random.default_rng(L + n)
    ref, qry = d.ref_seqs.copy(), d.query_seqs.copy()
    ref[rng.random(ref.shape) < 0.3] = ord('-')
    qry[:, : L // 2][rng.random((len(qry), L // 2)) < 0.5] = ord('-')
    nodes = np.array([d.tree.name_to_node[x] for x in d.ref_names], np.int32)
    groups = sorted(treecluster.grouped(d.tree, 0.3), key=lambda g: len(g[1]))
    small = groups.pop(next(i for i, g in enumerate(groups) if len(g[1]) >= 6))[1]
    cuts = np.cumsum([0] + [1 + k % 3 for k in range(len(small))])
    groups += [('cut%d' % k, small[a:b]) for k, (a, b) in enumerate(zip(cuts, cuts[1:])) if a < len(small)]
    row = {x: i for i, x in enumerate(d.ref_names)}
    big = [row[x] for x in max(groups, key=lambda g: len(g[1]))[1]]
    assert len(big) > 64
    r = big[0]
    sites = rng.choice(np.flatnonzero(ref[r] != ord('-')), 50, replace=False)
    if flagged:
        _sprinkle(ref, rng, 1 / 3)
        ref[r, sites] = ord('N')
    cons, rep_row, moff, mrow = ReducedReference(Alignment(d.ref_names, ref), False, groups).cluster_arrays()
    cons = cons.copy()
    if flagged:
        c = next(c for c in range(len(moff) - 1) if r in mrow[moff[c]:moff[c + 1]])
        _sprinkle(cons, np.random.default_rng(7), 1 / 3, keep=[0, c], rate=8 / L)  # (at most 16 in a row: the route's bound, api.hip)
        cons[c, sites[:8]] = ord('N')
        assert (~np.isin(cons, ACGT)).sum(axis=1).max() <= 16
    near = qry[20:40]
    near[:] = d.ref_seqs[r]  # (without the row's gaps: enough valid sites at overlap=0.52 too)
    near[(rng.random(near.shape) < 0.03) & np.isin(near, ACGT[:4])] = ord('A')
    _sprinkle(qry[10:110], np.random.default_rng(8))
    qry[10:110, L - 1] = ord('?')
    if flagged:
        qry[20:30, sites], qry[30:40, sites] = ord('N'), ord('n')
    if edge:
        qry[12] = ord('N')
        qry[13][~np.isin(qry[13], ACGT)] = ord('-')
        qry[13, L - 1] = ord('?')
    self_rows = None
    if own:
        bad = (~np.isin(ref, ACGT)).any(axis=1)
        rows = np.concatenate([np.flatnonzero(~bad)[100:192], np.flatnonzero(bad)[40:48]])
        self_rows = np.full(len(qry), -1, np.int32)
        qry[150:250], self_rows[150:250] = ref[rows], rows
    return d.tree, ref, qry, nodes, (cons, rep_row, moff, mrow), self_rows


@functools.lru_cache(maxsize=None)
def _oracle(inputs, kw=(), mode=None):
    """The C oracle on the table the engine builds (Engine._lut).  mode 'gaps': the queries' such bytes read as gaps; 'nN': their n as N."""
    tree, ref, qry, nodes, ca, self_rows = _inputs(*inputs)
    qry = qry.copy()
    if mode == 'gaps':
        qry[~np.isin(qry, ACGT)] = ord('-')
    if mode == 'nN':
        qry[qry == ord('n')] = ord('N')
    co = COracle(tree, ref, nodes, clusters=ca, method='OLS', criterion='MLSE', lut=jc69_lut(ref.shape[1], dict(kw).get('overlap', 0.001)),
                 threads=len(os.sched_getaffinity(0)), **dict(kw))
    return co.place_sequences(*((qry,) if self_rows is None else (qry, self_rows)))


def bite(inputs, kw=()):
    """On the oracle alone: the queries' such bytes matter, so does n against N, and a flagged query accepts the flagged big cluster."""
    want = _oracle(inputs, kw)
    assert _oracle(inputs, kw, 'gaps').tobytes() != want.tobytes()
    if inputs[2]:
        assert _oracle(inputs, kw, 'nN').tobytes() != want.tobytes()
        assert (want['n_obs'][20:40] > 64).any()
    return want


CASES = {
    'clean-context': dict(inputs=(1001, 600, False)),                  # D = 0, k1 only
    'k2-k3-k3x': dict(inputs=(1001, 600, True)),                       # the loosened representatives' screen with D > 1
    'all-N-and-ragged-word': dict(inputs=(1001, 600, True, True)),     # all-invalid pairs; the ragged word group
    'L5003': dict(inputs=(5003, 600, True)),                           # 13-bit counts near their top, G = 40
    'overlap': dict(inputs=(1001, 600, True), overlap=0.52),           # the window at the table's low end
    'own-rows-1200': dict(inputs=(1001, 1200, True, False, True)),     # lean sweep, clade blocks, flagged own rows
    'bit-count-form': dict(inputs=(1001, 600, True), debug=('no_cluster_mfma',)),
    'bit-count-flagged-tiles': dict(inputs=(1001, 600, True), knobs={'APPLES_CLUSTER_QX_BITCOUNT': 1}),  # k_cluster_dist_qx beside the matrix cores
    'matrix-core-flagged-tiles': dict(inputs=(1001, 600, True), knobs={'APPLES_CLUSTER_QX_MFMA': 1}),  # ... its second pass (k3 - k3x) on flagged clusters
    'knob-off': dict(inputs=(1001, 600, True), knobs={'APPLES_NO_CLUSTER_QUERY_EXOTIC': 1}),  # the 8-plane kernels as before: same bytes
}


@pytest.mark.parametrize('case', list(CASES), ids=str)
def test_placements_match_the_oracle(case):
    kw = dict(CASES[case])
    inputs, debug, knobs = kw.pop('inputs'), kw.pop('debug', ()), kw.pop('knobs', None)
    want = bite(inputs, tuple(sorted(kw.items())))
    tree, ref, qry, nodes, ca, self_rows = _inputs(*inputs)
    eng = Engine(tree, ref, nodes, clusters=ca, method='OLS', debug=debug, knobs=knobs, **kw)
    got = eng.place_sequences(*((qry,) if self_rows is None else (qry, self_rows)))
    info = eng.describe()
    assert np.array_equal(eng._lut, jc69_lut(ref.shape[1], kw.get('overlap', 0.001)))
    eng.close()
    assert info['code_planes'] == 2 and info['cluster_fused'] == 1, info
    off = 'APPLES_NO_CLUSTER_QUERY_EXOTIC' in (knobs or {})
    assert (info['cluster_query_exotic_fixes'] == 0) if off else (info['cluster_query_exotic_fixes'] >= 1), info
    assert off or (info['cluster_query_exotic_loosened_by'] > 1) == inputs[2], info
    assert info['cluster_blocks'] > 0 or len(ref) < 1024, info
    assert got.tobytes() == want.tobytes()
