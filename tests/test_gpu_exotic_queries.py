"""Query blocks in which many queries hold bytes beyond ACGT- (`N`, `.`, lower case: ordinary symbols to apples/distance.py:733-737)
stay on the fused matrix-core pass of a singleton JC69 context: the fp4 query image holds such bytes as gaps, the launch's screen is
loosened and k_query_exotic_fix gives every survivor its exact counts.  Byte for byte against the C oracle and against the route
without the fused pass.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import apples_oracle as orc  # noqa: E402
from oracle_c import COracle  # noqa: E402

from apples_amd import synth  # noqa: E402
from apples_amd.engine import Engine, jc69_lut  # noqa: E402

pytestmark = pytest.mark.gpu
NTHREADS = len(os.sched_getaffinity(0))
lut = functools.lru_cache(maxsize=None)(jc69_lut)

CASES = {
    'clean': dict(n=1500, L=200, nq=400),                              # k1 alone, D = 0: nothing loosened
    'dense': dict(n=1500, L=300, nq=500, dense=True, cap=8191),                # k2, k3, k3x; an exact match through matching such bytes
    'loosening-pair': dict(n=1500, L=300, nq=500, dense=True, pair=True, cap=8191),  # the screen's + D
    'overlap-rule': dict(n=1200, L=400, nq=300, dense=True, V=0.5, gap_rate=0.3, runs=True, cap=8191),  # the table's lower end
    'mfma-clean': dict(n=600, L=4100, nq=96),                          # k_jc69_mfma's survivors, 13-bit counts
    'mfma-dense': dict(n=600, L=4100, nq=96, dense=True, cap=8191),
    'streamed': dict(n=1500, L=200, nq=400, first=300, max_batch=64),  # the flags arrive after earlier chunks ran
}


def plant(q, ref, rng, dense=False, runs=False, first=0):
    """bytes beyond ACGT- into the queries from `first` on (q is changed in place)"""
    L = q.shape[1]
    t = q[first:]
    t[::2, 5] = ord('.')
    t[1::4, L - 10:] = ord('N')
    t[3::7] |= 0x20                      # lower case (`-` stays what it is)
    if dense:                            # over the rows' own runs of `.`: equal bytes, different bytes, a copy of a flagged row
        t[8::16, :L // 8] = ord('.')
        t[9::16, L - L // 8:] = ord('N')
        t[6] = ref[11]
    if runs:
        for i in range(0, len(t), 2):
            a = rng.integers(0, L - 120)
            t[i, a:a + rng.integers(60, 121)] = ord('N')


@pytest.mark.parametrize('case', list(CASES))
def test_query_blocks_with_bytes_beyond_acgt_stay_on_the_matrix_cores(case):
    c = {**dict(dense=False, pair=False, runs=False, V=0.001, gap_rate=0.05, first=0, max_batch=0, cap=None), **CASES[case]}
    n, L, nq, V = c['n'], c['L'], c['nq'], c['V']
    rng = np.random.default_rng(33)
    d = synth.make_dataset(n, L, nq, gap_rate=c['gap_rate'])
    nodes = np.array([d.tree.name_to_node[x] for x in d.ref_names], np.int32)
    ref = d.ref_seqs.copy()
    if c['dense']:                       # (tests/test_gpu_shapes.py: the dense form)
        for i in range(n):
            a, b = rng.integers(0, L // 6, size=2)
            ref[i, :a] = ord('.'); ref[i, L - b:] = ord('.')
            ref[i, rng.integers(0, L, size=3)] = ord('?')
    q = d.query_seqs.copy()
    plant(q, ref, rng, c['dense'], c['runs'], c['first'])
    if c['pair']:
        # a pair the pass alone would drop and the rule keeps: row 40 holds `.` on 100 of its 300 sites and letters elsewhere, query 2
        # copies it and changes 40 of the 200 letters.  The pass sees (200, 40), the rule (300, 40): the matching `.` count.
        ref[40] = np.where(d.ref_seqs[40] == ord('-'), ord('A'), d.ref_seqs[40])
        ref[40, 100:200] = ord('.')
        q[2] = ref[40]
        q[2, :40] = np.where(q[2, :40] == ord('A'), ord('C'), ord('A'))
        assert orc.jc69_from_counts(40, 200, L, V) > 0.2 >= orc.jc69_from_counts(40, 300, L, V) >= 0
    # (cap: the default keeps queries that would loosen the screen by more than 1 off the route -- it is slower than the 8-plane pass at
    # 200 000 leaves; the knob lifts the cap so that the loosened route itself is what these small shapes check)
    eng = Engine(d.tree, ref, nodes, method='OLS', overlap=V, max_batch=c['max_batch'],
                 knobs={'APPLES_QUERY_EXOTIC_CAP': c['cap']} if c['cap'] else None)
    got = eng.place_sequences(q)
    info = eng.describe()
    assert info['code_planes'] == 2 and info['eight_plane_copy'] == 1 and info['fused_distance_pass'].startswith('fp4'), info
    assert info['query_exotic_fixes'] > 0, info
    if c['first']:                       # the same block resident: the flags are known before the pass
        h, m = eng.upload_queries(q)
        eng.place_resident(h)
        assert eng.fetch(h, m).tobytes() == got.tobytes()
        eng.free_queries(h)
    eng.close()
    want = COracle(d.tree, ref, nodes, method='OLS', overlap=V, lut=lut(L, V), threads=NTHREADS).place_sequences(q)
    assert got.tobytes() == want.tobytes(), (case, info['query_exotic_loosened_by'], int((got['edge'] != want['edge']).sum()))
    e2 = Engine(d.tree, ref, nodes, method='OLS', overlap=V, max_batch=c['max_batch'], debug=('no_fuse',))
    assert e2.place_sequences(q).tobytes() == got.tobytes()
    e2.close()


def test_queries_beyond_the_cap_leave_the_route():
    """APPLES_QUERY_EXOTIC_CAP = 4 beside a reference row with 12 such bytes: a few queries with more such bytes are placed as a block of their own by the 8-plane kernels while
    the rest stays on the matrix cores; many of them send the whole block to the 8-plane kernels as before -- no launch of the new kernel."""
    d = synth.make_dataset(1500, 200, 400)
    nodes = np.array([d.tree.name_to_node[x] for x in d.ref_names], np.int32)
    ref = d.ref_seqs.copy()
    ref[3, 20:32] = ord('.')
    co = COracle(d.tree, ref, nodes, method='OLS', lut=lut(200, 0.001), threads=NTHREADS)
    eng = Engine(d.tree, ref, nodes, method='OLS', knobs={'APPLES_QUERY_EXOTIC_CAP': 4})
    q = d.query_seqs.copy()
    q[::2, 5] = ord('.')
    q[7:12, 190:] = ord('N')             # five queries beyond the cap
    assert eng.place_sequences(q).tobytes() == co.place_sequences(q).tobytes()
    fixes = eng.describe()['query_exotic_fixes']
    assert fixes > 0
    q[1::4, 190:] = ord('N')             # a quarter of the block beyond the cap
    assert eng.place_sequences(q).tobytes() == co.place_sequences(q).tobytes()
    assert eng.describe()['query_exotic_fixes'] == fixes
    eng.close()
