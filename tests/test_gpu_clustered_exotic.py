"""Clustered JC69 references with bytes beyond ACGT- (N . ? * n) stay on the fused route by representatives (csrc/select.hip:
k_cluster_dist_mfma's EX form, k_cluster_rep_fix, the k term), byte for byte against the C oracle.  Needs an MI355X."""
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
EX, ACGT = np.frombuffer(b'N.?*n', np.uint8), np.frombuffer(b'ACGT-', np.uint8)


def _sprinkle(rows, rng, keep=()):
    """Such bytes at about 1 % of the sites of about a third of the rows (never in the rows `keep`); which rows got one."""
    at = (rng.random(len(rows)) < 1 / 3)[:, None] & (rng.random(rows.shape) < 0.01)
    at[list(keep)] = False
    rows[at] = rng.choice(EX, int(at.sum()))
    return at.any(axis=1)


@functools.lru_cache(maxsize=None)
def _inputs(L=1001, n=600, reps=True, nq_ex=0, plain=False):
    """tests/test_gpu_long_alignments_clustered.py's rows and groups.  reps / nq_ex: consensus rows / that many queries carry such bytes too; plain: each replaced by a gap ('ctx': in the context alone)."""
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
    clean = [row[x] for x in next(g for g in groups if 2 <= len(g[1]) <= 32)[1]]  # one cluster stays clean, and the row query 8 copies
    bad = _sprinkle(ref, rng, keep=clean + [3])
    one = row[next(g for g in groups if len(g[1]) == 1)[1][0]]  # a flagged singleton cluster
    ref[one, 5], bad[one] = ord('N'), True
    qry[7], qry[8] = ord('-'), ref[3]
    cons, rep_row, moff, mrow = ReducedReference(Alignment(d.ref_names, ref), False, groups).cluster_arrays()
    cons = cons.copy()
    rep_bad = _sprinkle(cons, np.random.default_rng(7), keep=[0]) if reps else np.zeros(len(cons), bool)
    _sprinkle(qry[10:10 + nq_ex], np.random.default_rng(8))
    qry[10:10 + nq_ex, L - 1] = ord('?')
    flagged = [bad[mrow[a:b]].any() for a, b in zip(moff, moff[1:])]
    sizes = np.diff(moff)
    assert any(f and s > 64 for f, s in zip(flagged, sizes)) and any(f and s == 1 for f, s in zip(flagged, sizes)) and not all(flagged)
    assert rep_bad.any() == reps and not rep_bad.all()
    if plain:
        for x in (ref, cons, qry)[:2 if plain == 'ctx' else 3]:
            x[~np.isin(x, ACGT)] = ord('-')
    return d.tree, ref, qry, nodes, (cons, rep_row, moff, mrow)


@functools.lru_cache(maxsize=None)
def _oracle(inputs=(), kw=(), own_rows=False):
    """The C oracle on the table the engine builds for this length and overlap (Engine._lut)."""
    tree, ref, qry, nodes, ca = _inputs(*inputs)
    kw = dict(kw)
    co = COracle(tree, ref, nodes, clusters=ca, method=kw.pop('method', 'OLS'), criterion=kw.pop('criterion', 'MLSE'),
                 lut=jc69_lut(ref.shape[1], kw.get('overlap', 0.001)), threads=len(os.sched_getaffinity(0)), **kw)
    return co.place_sequences(*(_own_rows(inputs) if own_rows else (qry,)))


def _own_rows(inputs):
    """100 queries are reference rows placed without their own row: eight of them flagged members, their such bytes turned into gaps
    (a query with such a byte leaves the fused route); ten more equal a row, two of those rows flagged (an ex_block)."""
    _, ref, qry, _, _ = _inputs(*inputs)
    bad = (~np.isin(ref, ACGT)).any(axis=1)
    rows = np.concatenate([np.flatnonzero(~bad)[100:192], np.flatnonzero(bad)[40:48], np.flatnonzero(~bad)[200:208], np.flatnonzero(bad)[60:62]])
    qry, self_rows = qry.copy(), np.full(len(qry), -1, np.int32)
    qry[100:210] = ref[rows]
    qry[100:200][~np.isin(qry[100:200], ACGT)] = ord('-')
    self_rows[100:200] = rows[:100]
    return qry, self_rows


def _check(inputs=(), debug=(), own_rows=False, **kw):
    tree, ref, qry, nodes, ca = _inputs(*inputs)
    eng = Engine(tree, ref, nodes, clusters=ca, **{'knobs' if isinstance(debug, dict) else 'debug': debug, 'method': 'OLS', **kw})
    got = eng.place_sequences(*(_own_rows(inputs) if own_rows else (qry,)))
    info = eng.describe()
    assert np.array_equal(eng._lut, jc69_lut(ref.shape[1], kw.get('overlap', 0.001)))
    eng.close()
    assert info['code_planes'] == 2 and info['cluster_fused'] == 1 and info['cluster_exotic_clusters'] > 0 and info['eight_plane_copy'] == 1, info
    assert info['cluster_blocks'] > 0 or len(ref) < 1024 or 'no_blocks' in debug, info
    assert info['ragged_rows'] == isinstance(debug, dict), info  # (the ex_block left the main pass's ragged rows as they were)
    want = _oracle(inputs, tuple(sorted(kw.items())), own_rows)
    assert got.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize('L,reps,nq_ex', [(1001, False, 0), (1001, True, 0), (1001, True, 3), (1001, True, 100), (5003, True, 0)])
def test_placements_match_the_oracle(L, reps, nq_ex):
    """Members only; consensus rows too; 3 of 300 queries with such bytes (ex_block) and 100 (exact8); 13-bit counts near their top."""
    want = _check((L, 600, reps, nq_ex))
    assert want['n_obs'][7] == 0 and (want['n_obs'] > 64).any()  # (the all-gap query; a cluster of more than 64 members was accepted)
    assert _oracle((L, 600, reps, nq_ex, True)).tobytes() != want.tobytes()  # the recount matters


@pytest.mark.parametrize('kw', [dict(threshold=0.02, baseobs=25), dict(overlap=0.52), dict(method='FM', criterion='HYBRID')], ids=str)
def test_rules_and_records(kw):
    """Phase 4 and the slow list; valid / L about 0.525: the loosened table, every survivor tested again; the per-edge records."""
    _check(**kw)


@pytest.mark.parametrize('debug', [(), ('no_cluster_mfma',), ('no_blocks',), {'APPLES_RAGGED_SMALL': 64}], ids=str)
def test_clade_blocks_with_flagged_members(debug):
    """1 200 leaves: the lean sweep and the clade blocks; own rows and exact matches, flagged members among them; the bit-count form;
    ragged rows (by default from 65 536 reference rows), which the ex_block reads as plain full rows."""
    want = _check((1001, 1200), debug=debug, own_rows=True)
    assert (want['flags'][200:210] & 1).all() and not (want['flags'][100:192] & 1).any()  # F_EXACT (192..199, with gaps for such bytes, may equal a sibling row)


def test_a_query_block_with_such_bytes_keeps_the_panels():
    """A clean context, a clean block, then a block whose queries carry such bytes: nothing is re-packed, no panel is freed."""
    clean, ex = (1001, 600, True, 0, True), (1001, 600, True, 3, 'ctx')
    tree, ref, qry, nodes, ca = _inputs(*clean)
    eng = Engine(tree, ref, nodes, clusters=ca, method='OLS')
    got, got2, info = eng.place_sequences(qry), eng.place_sequences(_inputs(*ex)[2]), eng.describe()
    eng.close()
    assert info['cluster_fused'] == 1 and info['code_planes'] == 2 and info['eight_plane_copy'] == 1, info
    assert got.tobytes() == _oracle(clean).tobytes() and got2.tobytes() == _oracle(ex).tobytes()
