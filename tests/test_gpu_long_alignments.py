"""Alignments of 8 192 to 65 535 sites: the fused JC69 pass of singleton ACGT- contexts is the K-split fp4 GEMM
(csrc/dist_gemm.hip: k_jc69_gemm_long).  Placements are compared byte for byte with the C oracle without a distance table (libm's log, the
device's bits).  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle_c import COracle  # noqa: E402

from apples_amd import synth  # noqa: E402
from apples_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = 3840  # sites per split of the K loop (csrc/common.h GEMM_SPLIT_STEPS * 64)


@functools.lru_cache(maxsize=2)
def _inputs(L):
    """600 leaves x 300 queries (three reference tiles, a ragged query tile; 320 leaves at the top of the range): 30 % gaps in
    every reference row, half-gapped first halves of the queries, an all-gap query, an exact copy of a reference row, and a
    gap-free reference row with a query that differs from it at every 7th site (valid = L, d ~ 0.16: a survivor that carries
    the full-width counts; 29 more gap-free rows close to it, so that the query is placed from such survivors alone)."""
    d = synth.make_dataset(320 if L > 60000 else 600, L, 300, seed_tree=11, seed_aln=12, seed_query=13)
    rng = np.random.default_rng(L)
    ref, qry = d.ref_seqs.copy(), d.query_seqs.copy()
    full = ref[5].copy()
    ref[rng.random(ref.shape) < 0.3] = ord('-')
    qry[:, : L // 2][rng.random((len(qry), L // 2)) < 0.5] = ord('-')
    qry[7] = ord('-')
    qry[8] = ref[3]
    full[full == ord('-')] = ord('A')
    for k in range(30):  # (30 such rows, 29 of them a further 40th of the sites away: more survivors than the top-up rule asks for)
        ref[5 + k] = full
        if k:
            ref[5 + k, k::40] = np.where(full[k::40] == ord('G'), ord('T'), ord('G'))
    qry[9] = full
    qry[9, ::7] = np.where(full[::7] == ord('A'), ord('C'), ord('A'))
    nodes = np.array([d.tree.name_to_node[n] for n in d.ref_names], np.int32)
    return d.tree, ref, qry, nodes


def _oracle(L, qry=None, lut=None, **kw):
    tree, ref, q, nodes = _inputs(L)
    co = COracle(tree, ref, nodes, method='OLS', criterion='MLSE', lut=lut, threads=len(os.sched_getaffinity(0)), **kw)
    return co.place_sequences(q if qry is None else qry)


@pytest.mark.parametrize('L', [8192, 8193, 3 * SPLIT, 3 * SPLIT + 1, 20000, 65535])
def test_k_split_pass_matches_the_oracle(L):
    """Two splits and a few steps; the same with a ragged last word; three splits' worth of sites (two folds and a last split of 62 steps); the same and a site; valid counts
    past 8 191 (the screen's table still in LDS); the top of the range (the table gathered from global memory).  Between them
    the three tail shapes of the K loop."""
    tree, ref, qry, nodes = _inputs(L)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE')
    info = eng.describe()
    assert info['code_planes'] == 2
    assert info['fused_distance_pass'] == 'fp4 gemm, k-split', info
    assert info['gemm_split_sites'] == SPLIT
    got = eng.place_sequences(qry)
    assert eng.describe()['k_split_launches'] >= 1  # (the kernel itself ran, not a quiet fall-back to the bit-plane one)
    eng.close()
    # (at 8 192 sites exactly the engine still tabulates its distances, with numpy's log: the oracle gets that table, as in every
    # test of a context with one; beyond, neither has a table)
    assert (eng._lut is None) == (L > 8192)
    want = _oracle(L, lut=eng._lut)
    assert want['n_obs'][9] >= 30 and want['n_obs'][7] == 0  # (the inputs are what the docstring says)
    assert got.tobytes() == want.tobytes()


def test_overlap_rule_and_top_up_at_a_tight_threshold():
    """valid / L of these inputs is about 0.525: with -V 0.52 pairs fall on both sides of the overlap rule, and with -f 0.05 most
    queries go through the top-up path (full rows from the bit-plane kernel)."""
    tree, ref, qry, nodes = _inputs(8193)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE', overlap=0.52, threshold=0.05)
    assert eng.describe()['fused_distance_pass'] == 'fp4 gemm, k-split'
    got = eng.place_sequences(qry)
    eng.close()
    assert got.tobytes() == _oracle(8193, overlap=0.52, threshold=0.05).tobytes()


def test_same_bytes_without_the_gemm_route():
    tree, ref, qry, nodes = _inputs(8193)
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE', debug=('no_dist_gemm',))
    assert not eng.describe()['fused_distance_pass'].startswith('fp4 gemm')
    got = eng.place_sequences(qry)
    assert eng.describe()['k_split_launches'] == 0
    eng.close()
    assert got.tobytes() == _oracle(8193).tobytes()


def test_query_block_with_a_symbol_beyond_acgt_widens_the_context():
    """A `?` in a later query block sends the whole context to the 8-plane route: the image is freed, both blocks still equal
    the oracle."""
    tree, ref, qry, nodes = _inputs(8193)
    qry2 = qry[::-1].copy()
    qry2[4, 100] = ord('?')
    eng = Engine(tree, ref, nodes, method='OLS', criterion='MLSE')
    got = eng.place_sequences(qry)
    before = eng.describe()
    assert before['code_planes'] == 2 and before['k_split_launches'] >= 1
    got2 = eng.place_sequences(qry2)  # (streamed: the pass runs on the 2-plane forms first, sees the flag, widens and runs again)
    info = eng.describe()
    got3 = eng.place_sequences(qry)
    after = eng.describe()
    eng.close()
    assert info['code_planes'] == 8 and not info['fused_distance_pass'].startswith('fp4'), info
    assert after['k_split_launches'] == info['k_split_launches']  # (the widened context no longer takes the route)
    assert got.tobytes() == got3.tobytes() == _oracle(8193).tobytes()
    assert got2.tobytes() == _oracle(8193, qry=qry2).tobytes()
