"""
Every instantiation of the seed-filter scan kernel (kvq_scan_bp) the launcher can pick -- 36 cells of seed length,
index stride, lane group and kernel family -- against the oracle, order-exact, on workloads that reach each cell the
way production does: through the configuration, the table and the head of the text (tests/kernel_matrix.py; that
each lands on its cell and is not vacuous is checked without a GPU in tests/test_kernel_dispatch.py).
"""
import os

import pytest

import kernel_matrix as KM
from kvarq_amd import scan, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# switches that move the scan off the cell its inputs give (tools/r4_alt_switches.sh runs the suite under them):
# the oracle comparison still holds, the dispatch assertions do not
OVERRIDES = ('KVQ_K', 'KVQ_STRIDE', 'KVQ_LG', 'KVQ_DENSE', 'KVQ_DBG', 'KVQ_TILE')


@pytest.fixture(scope='module')
def g():
    return synth.genome()


@pytest.mark.parametrize('cell', KM.CELLS, ids=KM.cell_id)
def test_scan_kernel_cell_matches_the_oracle(g, cell):
    w = KM.Workload(cell, g)
    k, stride, lg, dense = cell
    overridden = any(os.environ.get(v) for v in OVERRIDES)
    t = scan.Table(w.seqs, **w.cfg)
    if not overridden:
        assert t.seed_k == k
        assert not t.seeded[w.refused_n] and not t.seeded[w.refused_short] and sum(t.seeded) == len(w.seqs) - 4
    # (KVQ_K lowers the seed length: the index then takes shorter sequences)
    assert t.seeded == [t.seed_k > 0 and KM.seedable(q, t.seed_k, w.cfg['maxerrors']) for q in w.seqs]
    for i, text in enumerate(w.texts):
        o = O.scan_memory(text, w.seqs, fold=True, nthreads=16, **w.cfg)
        s = scan.Scanner(t)
        s.scan_host(text)
        r = s.finish()
        s.close()
        if not overridden:
            assert r['kernel'] == dict(k=k, stride=stride, lg=lg, dense=dense), (i, r['kernel'])
            # (the table holds sequences the seed index refuses: the exhaustive kernels serve those)
            assert r['path'] == dict(seeded=True, exhaustive=True, rescanned=False, tiles_rescanned=False), (i, r['path'])
        assert len(r['hits']) == len(o['hits']) >= 100, (i, len(r['hits']), len(o['hits']))
        assert tuple(r['hits']) == tuple(o['hits']), i
        assert r['hitseqs'] == o['hitseqs'], i
        st, ost = r['stats'], o['stats']
        assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], i
        assert st['readlengths'] == ost['readlengths'] and st['records_parsed'] == ost['records_parsed'], i
        assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], i
    t.close()
