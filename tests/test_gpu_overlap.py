"""The overlapped route of a multi-batch block (csrc/api.hip: run_block_main): the distance GEMM of device batch b + 1 on the front
stream -- from the second batch on in the form that shares the CU (csrc/dist_gemm.hip: launch_counts_gemm, share) -- beside
selection, top-up chain and sweep of batch b on the back stream.  Placements are compared byte for byte with the serial route
(APPLES_OVERLAP=0) and with the C oracle.  Needs an MI355X."""
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

N_LEAVES, L, N_QUERIES, BATCH = 2000, 500, 3500, 1024
BIG = 600  # observed leaves from which a query goes to a workgroup-sized sweep team in these tests (APPLES_BIG_THRESHOLD)
KNOBS = {'APPLES_BIG_THRESHOLD': BIG}


@functools.lru_cache(maxsize=1)
def _inputs():
    """2 000 leaves x 3 500 queries of 500 sites: with max_batch = 1 024 four device batches, the last one of 428 queries.  Every
    50th query is a random sequence (nothing within -f: the top-up chain gives it its 25 nearest); the generator's own queries
    observe from a few dozen to more than BIG leaves, so every batch has queries for the wavefront-sized teams, for the
    workgroup-sized teams and for the top-up chain (test_inputs_exercise_both_side_chains)."""
    d = synth.make_dataset(N_LEAVES, L, N_QUERIES, seed_tree=21, seed_aln=22, seed_query=23)
    rng = np.random.default_rng(24)
    qry = d.query_seqs.copy()
    far = np.arange(0, N_QUERIES, 50)
    qry[far] = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, (len(far), L))]
    nodes = np.array([d.tree.name_to_node[n] for n in d.ref_names], np.int32)
    return d.tree, d.ref_seqs, qry, nodes, d.ref_names


@functools.lru_cache(maxsize=1)
def _oracle():
    tree, ref, qry, nodes, _ = _inputs()
    co = COracle(tree, ref, nodes, method='OLS', criterion='MLSE', lut=jc69_lut(L, 0.001), threads=len(os.sched_getaffinity(0)))
    want = co.place_sequences(qry)
    want.setflags(write=False)
    return want


def _engine(overlap=None, max_batch=BATCH, **kw):
    tree, ref, _, nodes, _ = _inputs()
    knobs = dict(KNOBS)
    if overlap is not None:
        knobs['APPLES_OVERLAP'] = overlap
    return Engine(tree, ref, nodes, method='OLS', criterion='MLSE', max_batch=max_batch, knobs=knobs, **kw)


def test_inputs_exercise_both_side_chains():
    want = _oracle()
    for b in range(0, N_QUERIES, BATCH):
        n_obs = want['n_obs'][b:b + BATCH]
        assert (n_obs > BIG).any(), 'no query for the workgroup-sized teams in batch %d' % (b // BATCH)
        assert (n_obs == 25).any(), 'no query on the top-up chain in batch %d' % (b // BATCH)
        assert ((n_obs > 25) & (n_obs <= BIG)).any()


@pytest.mark.parametrize('n_queries, batches', [(N_QUERIES, 4), (2 * BATCH, 2)])
def test_host_buffer_path_matches_serial_route_and_oracle(n_queries, batches):
    """Four batches with a partial last one; exactly two."""
    qry = _inputs()[2]
    eng = _engine()
    got = eng.place_sequences(qry[:n_queries])
    info = eng.describe()
    got2 = eng.place_sequences(qry[:n_queries])  # (second call: both sets of buffers and their events once more)
    eng.close()
    assert info['fused_distance_pass'].startswith('fp4 gemm'), info
    assert info['overlap'] == 1 and info['overlap_batches'] == batches, info
    ser = _engine(overlap=0)
    want_serial = ser.place_sequences(qry[:n_queries])
    sinfo = ser.describe()
    ser.close()
    assert sinfo['overlap'] == 0 and sinfo['overlap_batches'] == 0, sinfo
    assert got.tobytes() == want_serial.tobytes()
    assert got2.tobytes() == got.tobytes()
    assert got.tobytes() == _oracle()[:n_queries].tobytes()


def test_resident_path_twice_on_one_context():
    qry = _inputs()[2]
    eng = _engine()
    handle, _ = eng.upload_queries(qry)
    eng.place_resident(handle)
    info = eng.describe()
    first = eng.fetch(handle, N_QUERIES).copy()
    eng.place_resident(handle)
    second = eng.fetch(handle, N_QUERIES).copy()
    t = eng.timing()
    eng.free_queries(handle)
    eng.close()
    assert info['overlap'] == 1 and info['overlap_batches'] == 4, info
    assert first.tobytes() == _oracle().tobytes()
    assert second.tobytes() == first.tobytes()
    assert t['dist_ms'] > 0 and t['select_ms'] > 0 and t['sweep_ms'] > 0 and t['dist_launches'] == 4


def test_forced_on_is_the_same_route():
    qry = _inputs()[2]
    eng = _engine(overlap=1)
    got = eng.place_sequences(qry)
    info = eng.describe()
    eng.close()
    assert info['overlap'] == 1 and info['overlap_batches'] == 4
    assert got.tobytes() == _oracle().tobytes()


def test_one_batch_block_stays_serial():
    qry = _inputs()[2]
    eng = _engine(overlap=1, max_batch=0)
    got = eng.place_sequences(qry)
    info = eng.describe()
    eng.close()
    assert info['overlap'] == 0 and info['overlap_batches'] == 0, info
    assert got.tobytes() == _oracle().tobytes()


def test_clustered_context_stays_serial():
    """Max-diameter clusters with consensus representatives (the command line's default route), three device batches: the same bytes
    whatever the knob says."""
    from apples_amd import treecluster
    from apples_amd.fasta import Alignment
    from apples_amd.reference import ReducedReference
    tree, ref, qry, nodes, names = _inputs()
    clusters = ReducedReference(Alignment(names, ref), False, treecluster.grouped(tree, 0.2 * 1.2)).cluster_arrays()
    assert len(clusters[1]) < N_LEAVES
    out = []
    for knob in (0, 1):
        eng = Engine(tree, ref, nodes, clusters=clusters, method='OLS', criterion='MLSE', max_batch=BATCH,
                     knobs=dict(KNOBS, APPLES_OVERLAP=knob))
        out.append(eng.place_sequences(qry[:2 * BATCH + 100]))
        info = eng.describe()
        eng.close()
        assert info['all_singleton'] == 0 and info['overlap'] == 0 and info['overlap_batches'] == 0, info
    assert out[0].tobytes() == out[1].tobytes()
