"""Alignments of 8 192 to 65 535 sites whose REFERENCE rows hold bytes beyond ACGT-: the context keeps its 2-plane rows and fp4
image, the fused pass stays the K-split GEMM (k_jc69_gemm_long, EX form) and k_long_exotic_fix counts the sites back from one mask
plane per flagged row.  Placements are compared byte for byte with the C oracle.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle_c import COracle  # noqa: E402

from apples_amd import synth  # noqa: E402
from apples_amd.engine import Engine, jc69_lut  # noqa: E402

pytestmark = pytest.mark.gpu
BUILT = 43  # the row built against the gap-free query 9


@functools.lru_cache(maxsize=2)
def _inputs(L):
    """The recipe of test_gpu_long_alignments.py (600 leaves x 300 queries, 30 % gaps, rows 5..34 gap-free and close to the
    gap-free query 9, query 8 a copy of row 3), then in the reference, rows 3 and 5..34 left alone: bytes from N.?*n at 1 % of the
    sites of a third of the rows; row 40 with a single N; row 41 with a run of N over its first 8 300 sites (more than the 64 x 128
    one trip of the fix kernel's cooperative loop covers); row 42 with such bytes in its last, ragged word; and row 43 = query 9
    with N at every 20th site that query 9 shares with it (4.3 % of the sites): p = (1/7) / 0.957 = 0.149 with those sites read as
    gaps, passes -f 0.2 (p <= 0.1755); p = 1/7 + 0.043 = 0.186 with them counted, fails."""
    d = synth.make_dataset(600, L, 300, seed_tree=11, seed_aln=12, seed_query=13)
    rng = np.random.default_rng(L)
    ref, qry = d.ref_seqs.copy(), d.query_seqs.copy()
    full = ref[5].copy()
    ref[rng.random(ref.shape) < 0.3] = ord('-')
    qry[:, : L // 2][rng.random((len(qry), L // 2)) < 0.5] = ord('-')
    qry[7] = ord('-')
    qry[8] = ref[3]
    full[full == ord('-')] = ord('A')
    for k in range(30):
        ref[5 + k] = full
        if k:
            ref[5 + k, k::40] = np.where(full[k::40] == ord('G'), ord('T'), ord('G'))
    qry[9] = full
    qry[9, ::7] = np.where(full[::7] == ord('A'), ord('C'), ord('A'))
    rows = np.flatnonzero((rng.random(len(ref)) < 1 / 3) & (np.arange(len(ref)) > BUILT))
    hit = rng.random((len(rows), L)) < 0.01
    ref[rows] = np.where(hit, rng.choice(np.frombuffer(b'N.?*n', np.uint8), hit.shape), ref[rows])
    ref[40, 1000] = ord('N')
    ref[41, :8300] = ord('N')
    ref[42, L - 3:] = np.frombuffer(b'?*n', np.uint8)
    sites = np.arange(1, L, 20)
    ref[BUILT] = full
    ref[BUILT, sites[sites % 7 != 0]] = ord('N')
    nodes = np.array([d.tree.name_to_node[n] for n in d.ref_names], np.int32)
    return d.tree, ref, qry, nodes


@functools.lru_cache(maxsize=None)
def _oracle(L, variant='', **kw):
    """variant 'gaps': row 43's N read as gaps; 'q3' / 'q100': the query block of test 3.  At 8 192 sites exactly the engine
    tabulates its distances: the oracle gets the same table."""
    tree, ref, qry, nodes = _inputs(L)
    if variant == 'gaps':
        ref = ref.copy()
        ref[BUILT][ref[BUILT] == ord('N')] = ord('-')
    co = COracle(tree, ref, nodes, method='OLS', criterion='MLSE', lut=jc69_lut(L, 0.001) if L == 8192 else None,
                 threads=len(os.sched_getaffinity(0)), **kw)
    return co.place_sequences(_marked(L, int(variant[1:])) if variant.startswith('q') else qry)


def _marked(L, n):  # the queries in reverse order, n of them with a byte beyond ACGT-
    q = _inputs(L)[2][::-1].copy()
    q[4:4 + n, 100] = ord('?')
    return q


@pytest.mark.parametrize('L', [8192, 8193, 3 * 3840 + 1, 20480])
def test_reference_with_such_bytes_stays_on_the_k_split_route(L):
    """The caller's table; a ragged word; three splits; the screen's table gathered from global memory."""
    (tree, ref, qry, nodes), want = _inputs(L), _oracle(L)
    # (the inputs are what the docstring says: the built row is observed by query 9 only with its N read as gaps)
    assert want['n_obs'][9] >= 30 and _oracle(L, 'gaps')['n_obs'][9] == want['n_obs'][9] + 1
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE')
    info = eng.describe()
    assert info['code_planes'] == 2 and info['eight_plane_copy'] == 1 and info['fused_distance_pass'] == 'fp4 gemm, k-split', info
    assert info['exotic_sites_max_per_row'] == min(L, 8300), info
    got, after = eng.place_sequences(qry), eng.describe()
    eng.close()
    assert (eng._lut is None) == (L > 8192) and after['k_split_launches'] >= 1 and after['k_split_exotic_fixes'] >= 1, after
    assert got.tobytes() == want.tobytes()


def test_overlap_rule_and_top_up_at_a_tight_threshold():
    """valid / L is about 0.525: with -V 0.52 the sites counted back move pairs across the overlap rule (the screen's loosened low
    end), and with -f 0.05 most queries take the top-up path, full rows over the 8-plane copy."""
    tree, ref, qry, nodes = _inputs(8193)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE', overlap=0.52, threshold=0.05)
    got, info = eng.place_sequences(qry), eng.describe()
    eng.close()
    assert info['fused_distance_pass'] == 'fp4 gemm, k-split' and info['k_split_exotic_fixes'] >= 1, info
    assert got.tobytes() == _oracle(8193, overlap=0.52, threshold=0.05).tobytes()


@pytest.mark.parametrize('n', [3, 100])
def test_query_blocks_with_such_bytes_leave_the_context_as_it_is(n):
    """3 such queries are placed as a block of their own, 100 send their whole block to the 8-plane forms; the context keeps its
    2-plane rows either way, and a clean block behind them runs on the K-split route."""
    tree, ref, qry, nodes = _inputs(8193)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE')
    got2, mid = eng.place_sequences(_marked(8193, n)), eng.describe()
    got, after = eng.place_sequences(qry), eng.describe()
    eng.close()
    assert mid['code_planes'] == after['code_planes'] == 2 and after['fused_distance_pass'] == 'fp4 gemm, k-split', after
    assert after['k_split_launches'] > mid['k_split_launches'] and after['k_split_exotic_fixes'] > mid['k_split_exotic_fixes']
    assert got2.tobytes() == _oracle(8193, 'q%d' % n).tobytes()
    assert got.tobytes() == _oracle(8193).tobytes()


def test_same_bytes_without_the_gemm_route():
    tree, ref, qry, nodes = _inputs(8193)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE', debug=('no_dist_gemm',))
    got, after = eng.place_sequences(qry), eng.describe()
    eng.close()
    assert not after['fused_distance_pass'].startswith('fp4 gemm') and after['k_split_launches'] == after['k_split_exotic_fixes'] == 0
    assert got.tobytes() == _oracle(8193).tobytes()
