"""
Every instantiation of the seed-filter scan kernel (kvq_scan_bp) the launcher can pick -- 36 cells of seed length,
index stride, lane group and kernel family -- against the oracle, order-exact, on workloads that reach each cell the
way production does: through the configuration, the table and the head of the text (tests/kernel_matrix.py; that
each lands on its cell and is not vacuous is checked without a GPU in tests/test_kernel_dispatch.py).

Each workload is scanned three times and every result held to the same comparison: in this process at the grid the
launcher gives (a workgroup then sees one or two of a text's 28..101 tiles), and in a child process each under
KVQ_GRID=1 and KVQ_GRID=5 (the switch is read once per process), where a workgroup walks all the tiles or a fifth of
them: it draws the tile after next from its own share, goes through the other shares in its own order when that has
run out -- at 5 racing the others for a share's last tile -- and carries its record count, its longest read, its
chunk of the survivors' list and its planes in LDS from tile to tile.  ``r['grid']`` says that the switch was taken.
KM.long_walk() is the text for what no matrix text reaches: a share of four and more tiles, and the flush of a
workgroup's read-length histogram after 100 tiles.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import kernel_matrix as KM
from kvarq_amd import scan, synth
from kvarq_amd.engine import Hit
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# switches that move the scan off the cell its inputs give (tools/r4_alt_switches.sh runs the suite under them):
# the oracle comparison still holds, the dispatch assertions do not
OVERRIDES = ('KVQ_K', 'KVQ_STRIDE', 'KVQ_LG', 'KVQ_DENSE', 'KVQ_DBG', 'KVQ_TILE')

GRIDS = (1, 5)              # KVQ_GRID of the children
CHILD_LIMIT = 120           # seconds a child may take (the longest one seen: the docstring of run_children)
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'grid_child.py')
SEEDED_AND_EXHAUSTIVE = dict(seeded=True, exhaustive=True, rescanned=False, tiles_rescanned=False)
SEEDED_ALONE = dict(seeded=True, exhaustive=False, rescanned=False, tiles_rescanned=False)


@pytest.fixture(scope='module')
def g():
    return synth.genome()


def switched():
    """(a switch moves the scan off its cell, KVQ_GRID is set here already)"""
    return any(os.environ.get(v) for v in OVERRIDES), os.environ.get('KVQ_GRID')


def compare(r, o, what, cell=None, path=None, grid=None, min_hits=100):
    """one scan's result against the oracle's: hits order-exact, hit bytes, the four statistics, coverage and mutations;
    the kernel that ran, the path the batch took and the workgroups of the launch where they are given"""
    if cell is not None:
        k, stride, lg, dense = cell
        assert r['kernel'] == dict(k=k, stride=stride, lg=lg, dense=dense), (what, r['kernel'])
    if path is not None:
        assert r['path'] == path, (what, r['path'])
    if grid is not None:
        assert r['grid'] == grid, (what, r['grid'], grid)
    assert len(r['hits']) == len(o['hits']) >= min_hits, (what, len(r['hits']), len(o['hits']))
    assert tuple(r['hits']) == tuple(o['hits']), what
    assert r['hitseqs'] == o['hitseqs'], what
    st, ost = r['stats'], o['stats']
    assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], what
    assert st['readlengths'] == ost['readlengths'] and st['records_parsed'] == ost['records_parsed'], \
        (what, [(i, a, b) for i, (a, b) in enumerate(zip(st['readlengths'], ost['readlengths'])) if a != b][:8], st['records_parsed'], ost['records_parsed'])
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], what


def run_children(tmp_path, texts, seqs, cfg, what):
    """{grid: [what Scanner.finish gave for each text]} from one child process per grid in GRIDS, one after the other.

    A child is a GPU step of its own with a time limit of its own.  One that ends by a signal, aborts or runs into the
    limit ends the session: nothing more is started on the GPU behind it, and nothing is tried again.  (The longest child
    seen on an MI355X took 0.7 s, all 76 of the suite 32 s together: starting Python and the device is most of it.)"""
    files = []
    for i, text in enumerate(texts):
        files.append(str(tmp_path / ('t%d.fastq' % i)))
        text.tofile(files[-1])
    out = {}
    for grid in GRIDS:
        res = str(tmp_path / ('grid%d.npz' % grid))
        job = str(tmp_path / ('grid%d.json' % grid))
        with open(job, 'w') as f:
            json.dump(dict(texts=files, seqs=[q.decode('latin-1') for q in seqs], cfg=cfg, result=res), f)
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, CHILD, job], env=dict(os.environ, KVQ_GRID=str(grid)),
                               capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired as e:
            pytest.exit('%s, KVQ_GRID=%d: the child did not end within %d s\n%s\n%s' % (what, grid, CHILD_LIMIT, e.stdout, e.stderr), 1)
        print('%s, KVQ_GRID=%d: child took %.1f s' % (what, grid, time.time() - t0))
        said = p.stdout + p.stderr
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
            pytest.exit('%s, KVQ_GRID=%d: the child ended with status %d\n%s' % (what, grid, p.returncode, said), 1)
        assert p.returncode == 0 and 'grid child ok' in p.stdout, (what, grid, said)
        z = np.load(res)
        out[grid] = []
        for i in range(len(texts)):
            a = lambda name: z['t%d_%s' % (i, name)]
            off, blob = a('offsets').tolist(), a('blob').tobytes()
            meta = json.loads(str(a('meta')))
            cols = [a(c).tolist() for c in ('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')]
            out[grid].append(dict(
                hits=tuple(Hit(*h) for h in zip(*cols)), hitseqs=[blob[x:y] for x, y in zip(off[:-1], off[1:])],
                stats=dict(nseqhits=tuple(a('nseqhits').tolist()), nseqbasehits=tuple(a('nseqbasehits').tolist()),
                           readlengths=tuple(a('readlengths').tolist()), records_parsed=int(a('records_parsed'))),
                coverage=a('coverage'), mutations=a('mutations'), kernel=meta['kernel'], path=meta['path'], grid=meta['grid']))
    return out


@pytest.mark.parametrize('cell', KM.CELLS, ids=KM.cell_id)
def test_scan_kernel_cell_matches_the_oracle(g, cell, tmp_path):
    w = KM.Workload(cell, g)
    k, stride, lg, dense = cell
    overridden, grid_env = switched()
    t = scan.Table(w.seqs, **w.cfg)
    if not overridden:
        assert t.seed_k == k
        assert not t.seeded[w.refused_n] and not t.seeded[w.refused_short] and sum(t.seeded) == len(w.seqs) - 4
    # (KVQ_K lowers the seed length: the index then takes shorter sequences)
    assert t.seeded == [t.seed_k > 0 and KM.seedable(q, t.seed_k, w.cfg['maxerrors']) for q in w.seqs]
    small = run_children(tmp_path, w.texts, w.seqs, w.cfg, KM.cell_id(cell)) if not (overridden or grid_env) else {}
    for i, text in enumerate(w.texts):
        o = O.scan_memory(text, w.seqs, fold=True, nthreads=16, **w.cfg)
        tiles = sum(KM.tiles_of(text)[1])
        s = scan.Scanner(t)
        s.scan_host(text)
        r = s.finish()
        s.close()
        # (the table holds sequences the seed index refuses: the exhaustive kernels serve those)
        compare(r, o, (i, 'in process'), cell if not overridden else None, SEEDED_AND_EXHAUSTIVE if not overridden else None,
                min(int(grid_env), tiles) if grid_env and not overridden else None)
        assert overridden or 1 <= r['grid'] <= tiles, (i, r['grid'], tiles)
        for grid in sorted(small):
            compare(small[grid][i], o, (i, 'KVQ_GRID=%d' % grid), cell, SEEDED_AND_EXHAUSTIVE, min(grid, tiles))
    t.close()


@pytest.mark.parametrize('n', range(len(KM.LongWalk.CELLS)), ids=['k5-drain', 'k8-halve'])
def test_a_workgroup_that_walks_hundreds_of_tiles_matches_the_oracle(g, n, tmp_path):
    """KM.long_walk(): 272 tiles of about 452 records, every share of them four tiles or more, no sequence and no record
    for any kernel but the seed-filter scan.  Under KVQ_GRID=1 one workgroup flushes its read-length histogram behind
    tile 100 and tile 200 with some 45 000 counts in the bin of 40 and goes through all 64 shares; under KVQ_GRID=5 five
    do a fifth each and meet at the ends of the shares."""
    w = KM.long_walk(g)
    cell, cfg = w.CELLS[n], w.cfgs[n]
    overridden, grid_env = switched()
    o = O.scan_memory(w.text, w.seqs, fold=True, nthreads=16, **cfg)
    tiles = sum(KM.tiles_of(w.text)[1])
    small = run_children(tmp_path, [w.text], w.seqs, cfg, 'long walk ' + KM.cell_id(cell)) if not (overridden or grid_env) else {}
    t = scan.Table(w.seqs, **cfg)
    s = scan.Scanner(t)
    s.scan_host(w.text)
    r = s.finish()
    s.close()
    t.close()
    compare(r, o, 'in process', cell if not overridden else None, SEEDED_ALONE if not overridden else None,
            min(int(grid_env), tiles) if grid_env and not overridden else None, min_hits=500)
    assert overridden or 1 <= r['grid'] <= tiles, (r['grid'], tiles)
    for grid in sorted(small):
        compare(small[grid][0], o, 'KVQ_GRID=%d' % grid, cell, SEEDED_ALONE, min(grid, tiles), min_hits=500)
