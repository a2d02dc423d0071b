"""
The two bodies of a tile in the seed-filter scan kernel (kvq_scan_bp, kernels_bp_pass.inc), order-exact against the
oracle like tests/test_gpu_kernel_matrix.py.  A kernel with a fixed lane group runs a tile of at most RP = 512 >> LG
records as ONE pass of ONE stretch per wave with ONE window of work items, straight through; a wave leaves that body
for the loops when a candidate queue overflows or its work items outgrow their window, and a tile of more than RP
records, the draining kernels and the kernel that works the lane group out per tile know the loops only.  The texts
here sit on those seams:

* tiles of RP - 1, RP and RP + 1 records in one text, for every fixed lane group (forced with KVQ_LG),
* a read that floods its wave's candidate queue (the stretch is halved down to that read, which goes to the redo
  list) in a tile's only pass and in the second pass of a tile of three, and a read whose work items outgrow their
  window,
* header lines so long that a tile's first ten newlines do not lie in wave 0's stretch (P2's general form), chunks
  whose ends are not 16-byte aligned (the planes are cut in place) and the speculated tile next to a chunk's first,
* one workgroup that carries its state through all of that (KVQ_GRID=1), and the same text through the draining
  kernels (KVQ_DENSE=1, KVQ_K=6), which kept the loops.

Runs that need a launcher switch are children (tests/grid_child.py: the switches are read once per process); every
run's reported kernel and grid are asserted, so a switch that was not taken fails.
"""
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import kernel_matrix as KM
from kvarq_amd import _lib, scan, synth
from kvarq_amd.engine import Hit
from oracle import oracle as O

pytestmark = pytest.mark.gpu

OVERRIDES = ('KVQ_K', 'KVQ_STRIDE', 'KVQ_LG', 'KVQ_DENSE', 'KVQ_DBG', 'KVQ_TILE', 'KVQ_GRID')
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'grid_child.py')
CHILD_LIMIT = 120
CFG = dict(KM.CONFIGS[8])
WAVE0 = 80 * 64                 # bytes of a tile's window that wave 0 turns into planes (ST_BLK * 64)
BP_QW = BP_Q2W = 96             # candidates / work items a wave's queues hold


@pytest.fixture(scope='module')
def g():
    return synth.genome()


def overridden():
    return any(os.environ.get(v) for v in OVERRIDES)


def sparse_table(g):
    """40 SNP templates of 51 bases and their reverse complements: stride 8, nothing for the exhaustive kernels"""
    plus = [q for q in synth.table(g) if len(q) == 51][:40]
    return plus, synth.both_strands(plus)


def flood_table(g):
    """... plus a sequence of span_of(8, 2, 2) bases, which sets the stride to 2 (a 300-base read then has 147 lookups), and 40 A"""
    plus, _ = sparse_table(g)
    plus = plus + [g[2008200:2008200 + KM.span_of(8, CFG['maxerrors'], 2)].tobytes(), b'A' * 40]
    return plus, synth.both_strands(plus)


class Text(object):
    """records appended one by one; every eighth carries (a piece of) a template with 0..2 substitutions, every fifth a bad score or three"""

    def __init__(self, plus, seed):
        self.rng, self.plus, self.out, self.n, self.at, self.starts = random.Random(seed), plus, [], 0, 0, []

    def add(self, size=None, L=None, bases=None, name=None):
        """a record of `size` bytes (or of L bases / the given bases); returns its index"""
        rng = self.rng
        if bases is not None:
            L = len(bases)
        if name is None:
            nl = 7 if size is None or (size - 6 - 7) % 2 == 0 else 8
            name = (b'%x' % self.n).rjust(nl, b'r')
        if L is None:
            L = (size - 6 - len(name)) // 2
            assert 2 * L + 6 + len(name) == size and L > 0, (size, L)
        if bases is None:
            bases = KM._rand(rng, L)
            if self.n % 8 == 3:
                q = self.plus[rng.randrange(40)]
                m = min(L, len(q))
                a, at = rng.randrange(0, len(q) - m + 1), rng.randrange(0, L - m + 1)
                bases = bases[:at] + KM._mutate(rng, q[a:a + m], rng.sample(range(m), self.n // 8 % 3)) + bases[at + m:]
        quals = bytearray(b'I' * L)
        if self.n % 5 == 2:
            for _ in range(1 + self.n % 3):
                quals[rng.randrange(L)] = ord('#')
        r = b'@' + name + b'\n' + bases + b'\n+\n' + bytes(quals) + b'\n'
        self.starts.append(self.at); self.out.append(r); self.at += len(r); self.n += 1
        return self.n - 1

    def run(self, avg, until=None, n=None):
        """records of `avg` bytes on average (whole bytes each, the rounding carried along), n of them or up to offset `until`"""
        base, i = self.at, 0
        while (i < n) if n is not None else (self.at < until):
            self.add(size=int(round(base + (i + 1) * avg)) - self.at)
            i += 1

    def head(self, size):
        """the first 128 KiB and a little (they set the tile and the lane group): records of `size` bytes"""
        while self.at < (128 << 10) + 8192:
            self.add(size=size)
        return _lib.lib().kvq_tile_for_text(self.array().ctypes.data, 128 << 10, None)

    def array(self):
        return np.frombuffer(b''.join(self.out), dtype=np.uint8)


def layout(text, starts):
    """(tile bytes, tiles, [(chunk, tile of the chunk) of every record start], chunk offsets) as the launcher cuts a text scanned as ONE host batch"""
    tile, per_chunk = KM.tiles_of(text)
    co = [int(x) for x in scan.chunk_offsets(text)]
    where, c = [], 0
    for s in starts:
        while s >= co[c + 1]:
            c += 1
        where.append((c, (s - (co[c] & ~15)) // tile))
    return tile, sum(per_chunk), where, co


def records_per_tile(where):
    out = {}
    for w in where:
        out[w] = out.get(w, 0) + 1
    return out


def compare(r, o, what, kernel=None, grid=None, min_hits=20):
    """one scan's result against the oracle's: hits order-exact, hit bytes, the statistics, coverage and mutations; the kernel and the grid of the launch"""
    if kernel is not None:
        assert r['kernel'] == kernel, (what, r['kernel'], kernel)
    if grid is not None:
        assert r['grid'] == grid, (what, r['grid'], grid)
    assert len(r['hits']) == len(o['hits']) >= min_hits, (what, len(r['hits']), len(o['hits']))
    assert tuple(r['hits']) == tuple(o['hits']), what
    assert r['hitseqs'] == o['hitseqs'], what
    st, ost = r['stats'], o['stats']
    assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], what
    assert st['readlengths'] == ost['readlengths'] and st['records_parsed'] == ost['records_parsed'], \
        (what, [(i, a, b) for i, (a, b) in enumerate(zip(st['readlengths'], ost['readlengths'])) if a != b][:8], st['records_parsed'], ost['records_parsed'])
    assert list(np.asarray(r['coverage']).tolist()) == list(o['coverage']) and list(np.asarray(r['mutations']).tolist()) == list(o['mutations']), what


def in_process(text, seqs):
    t = scan.Table(seqs, **CFG)
    s = scan.Scanner(t)
    s.scan_host(text)
    r = s.finish()
    s.close()
    t.close()
    return r


def child(tmp_path, text, seqs, env, what):
    """what Scanner.finish gave for the text in a process of its own under the switches `env`.  A child is a GPU step of its own
    with a time limit of its own; one that ends by a signal, aborts or runs into the limit ends the session."""
    tag = '_'.join('%s%s' % kv for kv in sorted(env.items()))
    path, res, job = str(tmp_path / 't.fastq'), str(tmp_path / (tag + '.npz')), str(tmp_path / (tag + '.json'))
    text.tofile(path)
    with open(job, 'w') as f:
        json.dump(dict(texts=[path], seqs=[q.decode('latin-1') for q in seqs], cfg=CFG, result=res), f)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, job], env=dict(os.environ, **env), capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as e:
        pytest.exit('%s, %s: the child did not end within %d s\n%s\n%s' % (what, tag, CHILD_LIMIT, e.stdout, e.stderr), 1)
    print('%s, %s: child took %.1f s' % (what, tag, time.time() - t0))
    said = p.stdout + p.stderr
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
        pytest.exit('%s, %s: the child ended with status %d\n%s' % (what, tag, p.returncode, said), 1)
    assert p.returncode == 0 and 'grid child ok' in p.stdout, (what, tag, said)
    z = np.load(res)
    a = lambda name: z['t0_%s' % name]
    off, blob = a('offsets').tolist(), a('blob').tobytes()
    meta = json.loads(str(a('meta')))
    cols = [a(c).tolist() for c in ('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')]
    return dict(hits=tuple(Hit(*h) for h in zip(*cols)), hitseqs=[blob[x:y] for x, y in zip(off[:-1], off[1:])],
                stats=dict(nseqhits=tuple(a('nseqhits').tolist()), nseqbasehits=tuple(a('nseqbasehits').tolist()),
                           readlengths=tuple(a('readlengths').tolist()), records_parsed=int(a('records_parsed'))),
                coverage=a('coverage'), mutations=a('mutations'), kernel=meta['kernel'], path=meta['path'], grid=meta['grid'])


# ---------------------------------------------------------------------------
# RP - 1, RP, RP + 1 records a tile
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('lg', (2, 1, 3))
def test_tiles_of_one_record_less_and_more_than_a_pass_holds(g, lg, tmp_path):
    """Behind the head, fourteen tiles' worth of records of tile / (RP - 1/2) bytes -- tiles of RP - 1 and of RP records by turns,
    wherever the tiles begin -- and fourteen of tile / (RP + 1/2): RP and RP + 1.  A tile of RP records is the last the
    straight body takes; one of RP + 1 takes two turns of the pass loop, the second for a single record."""
    if overridden():
        pytest.skip('runs under launcher switches of its own')
    plus, seqs = sparse_table(g)
    RP = 512 >> lg
    tx = Text(plus, 100 + lg)
    tile = tx.head(int(round(39700.0 / (RP - 0.5))))
    tx.run(tile / (RP - 0.5), n=14 * RP)
    tx.run(tile / (RP + 0.5), n=14 * RP)
    text = tx.array()
    tile2, tiles, where, _ = layout(text, tx.starts)
    counts = set(records_per_tile(where).values())
    assert tile2 == tile and tiles <= 60 and {RP - 1, RP, RP + 1} <= counts, (tile, tile2, tiles, sorted(counts))
    o = O.scan_memory(text, seqs, fold=True, nthreads=16, **CFG)
    r = child(tmp_path, text, seqs, dict(KVQ_LG=str(lg)), 'lg %d' % lg)
    compare(r, o, 'KVQ_LG=%d' % lg, dict(k=8, stride=8, lg=lg, dense=False), tiles)


# ---------------------------------------------------------------------------
# queues that overflow, long headers, chunk ends: one text, every launch
# ---------------------------------------------------------------------------

class Seams(object):
    def __init__(self, g):
        self.plus, self.seqs = flood_table(g)
        e = CFG['maxerrors']
        assert KM.index_stride(self.seqs, 8, e) == 2 and not KM.index_dense(self.seqs, 8, e, 2)
        tx = Text(self.plus, 7)
        rng = tx.rng
        tile = tx.head(2 * 150 + 6 + 7)
        # a read of 300 A: 147 lookups that all meet the anchor block AAAAAAAA -- more candidates than BP_QW, whatever the stretch is halved to
        tx.run(313, until=tx.at + 3 * tile // 2)
        self.flood_one_pass = tx.add(bases=b'A' * 300)
        tx.run(313, until=tx.at + tile)
        # a read with 60 A in it: 27 candidates (below BP_QW) of six index entries each, and as many again for the other strand's T -- more work items than one window
        self.many_items = tx.add(bases=KM._rand(rng, 45) + b'A' * 60 + KM._rand(rng, 45))
        tx.run(313, until=tx.at + tile)
        # short records, three passes a tile; the flooding read among the records of a tile's second pass
        short0 = tx.n
        tx.run(2 * 50 + 6 + 7, until=tx.at + 5 * tile)
        short1 = tx.n
        tx.run(313, until=tx.at + tile)
        # header lines of 2100 bytes: ten newlines take more than wave 0's 5120 bytes
        self.long0 = tx.n
        for i in range(70):
            tx.add(L=150, name=(b'%d' % i).rjust(2100, b'h'))
        self.long1 = tx.n
        tx.run(313, until=2250000)                   # (chunks are cut every MiB: two cuts inside the text)
        # (the flooding read goes in last: what stands in front of it stays where it is)
        _, _, where, _ = layout(tx.array(), tx.starts)
        per, seen, at = records_per_tile(where), {}, None
        for i in range(short0, short1):
            seen[where[i]] = seen.get(where[i], 0) + 1
            if seen[where[i]] == 190 and per[where[i]] > 300 and where[i + 150] == where[i] and i > short0 + 400:
                at = i
                break
        assert at is not None
        flood = b'@flood\n' + b'A' * 300 + b'\n+\n' + b'I' * 300 + b'\n'
        tx.out.insert(at, flood)
        tx.starts = [s if i < at else s + len(flood) for i, s in enumerate(tx.starts)]
        tx.starts.insert(at, tx.starts[at] - len(flood))
        self.flood_second_pass = at
        shift = lambda i: i + 1 if i >= at else i
        self.long0, self.long1 = shift(self.long0), shift(self.long1)
        self.text = tx.array()
        self.starts = tx.starts
        self.tile, self.tiles, self.where, self.co = layout(self.text, self.starts)
        self.oracle = O.scan_memory(self.text, self.seqs, fold=True, nthreads=16, **CFG)


_seams = []


@pytest.fixture(scope='module')
def seams(g):
    if not _seams:
        _seams.append(Seams(g))
    return _seams[0]


def test_the_seams_text_holds_what_it_is_for(seams):
    """(the text is what the docstring of this module says; checked here, once, not in every run)"""
    w = seams
    per = records_per_tile(w.where)
    assert w.tiles <= 60 and w.text.nbytes <= 2400000, (w.tiles, w.text.nbytes)
    # the flooding reads: one in a tile of one pass, one among the records 129..256 of a tile of three passes
    assert per[w.where[w.flood_one_pass]] < 128
    wt = w.where[w.flood_second_pass]
    k = sum(1 for i in range(w.flood_second_pass) if w.where[i] == wt)
    assert 128 + 8 <= k < 256 - 8 and per[wt] > 2 * 128 + 8, (k, per[wt])
    raw = w.text.tobytes()
    assert raw[w.starts[w.flood_second_pass]:].startswith(b'@flood\n' + b'A' * 300 + b'\n')
    assert 60 // 2 * 6 > BP_Q2W and 60 // 2 < BP_QW < 300 // 2 - 4
    # header lines: a tile that begins among them sees fewer than ten newlines in its first 5120 bytes
    assert any(raw[a:a + WAVE0 - 80].count(b'\n') < 10 for a in [(w.co[c] & ~15) + t * w.tile for c, t in set(w.where[w.long0 + 8:w.long1 - 8])])
    # chunks: several, with first and last bytes that are not 16-byte aligned
    assert len(w.co) >= 4 and sum(1 for a in w.co[1:-1] if a & 15) >= 2, w.co
    assert len(w.oracle['hits']) >= 100


def test_overflowing_queues_long_headers_and_chunk_ends_in_process(seams):
    if overridden():
        pytest.skip('the launcher switches of the environment move the scan off its kernel')
    w = seams
    r = in_process(w.text, w.seqs)
    compare(r, w.oracle, 'in process', dict(k=8, stride=2, lg=2, dense=False), w.tiles, min_hits=100)
    assert r['path']['seeded'] and r['path']['exhaustive'], r['path']          # (the flooding reads went through the redo list)


@pytest.mark.parametrize('env,kernel', [
    (dict(KVQ_GRID='1'), dict(k=8, stride=2, lg=2, dense=False)),
    (dict(KVQ_DENSE='1'), dict(k=8, stride=2, lg=2, dense=True)),
    (dict(KVQ_K='6'), dict(k=6, stride=None, lg=2, dense=True)),
], ids=['grid1', 'dense', 'k6'])
def test_one_workgroup_and_the_draining_kernels_on_the_same_text(seams, env, kernel, tmp_path):
    """KVQ_GRID=1: one workgroup walks every tile, straight tiles and tiles of loops by turns, and carries its counts, its chunk of
    the survivors' list and its planes through them.  KVQ_DENSE=1, KVQ_K=6: the draining kernels, which have the loops only."""
    if overridden():
        pytest.skip('runs under launcher switches of its own')
    w = seams
    if kernel['stride'] is None:
        kernel = dict(kernel, stride=KM.index_stride(w.seqs, 6, CFG['maxerrors']))
    r = child(tmp_path, w.text, w.seqs, env, 'seams')
    compare(r, w.oracle, str(env), kernel, 1 if 'KVQ_GRID' in env else w.tiles, min_hits=100)
