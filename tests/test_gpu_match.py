"""
The matchers at the seams of their compare loops (tests/match_matrix.py; checked without a GPU in
tests/test_match_host.py): every spec record aims one alignment with exactly maxerrors or maxerrors + 1 mismatches,
one of them on a seam, at one sequence.  "Observed per alignment" means: beside the whole result equalling the
oracle's (hits in order, hit bytes, nseqhits, nseqbasehits, read lengths, coverage, mutations), the hits of every spec
record on its target equal what the plain statement of workhorse.c:1112-1174 planned for it, and a failure names the
spec.  Every route to a matcher is taken on purpose and asserted (``path``, ``Scanner.match_info()``, the kernel cell),
so that a test fails when its route was not taken instead of repeating the default run.  Bit-exact throughout.
"""
import os

import pytest

import match_matrix as MM
from kvarq_amd import scan
from oracle import oracle as O
from test_gpu_kernel_matrix import OVERRIDES, SEEDED_ALONE, SEEDED_AND_EXHAUSTIVE

pytestmark = pytest.mark.gpu

EXHAUSTIVE_ALONE = dict(seeded=False, exhaustive=True, rescanned=False, tiles_rescanned=False)
TEXTS = [(name, bg) for name in MM.CELLS for bg in MM.BACKGROUNDS[name]]

_oracle = {}


def oracle_of(name, bg, full):
    """one oracle run per text and table, shared by the tests that want it"""
    w = MM.cell(name)
    if (name, bg, full) not in _oracle:
        _oracle[name, bg, full] = O.scan_memory(w.texts[bg].data, w.seqs if full else w.seqs_kept, fold=True, nthreads=16, **w.cfg)
    return _oracle[name, bg, full]


def overridden():
    return any(os.environ.get(v) for v in OVERRIDES)


def check(r, o, text, nseq, where):
    # per spec: the statement's hits, no other and no less
    got, want = text.by_spec(r['hits']), text.planned(nseq)
    assert len(want) > len(text.specs) // 3
    for i, s in enumerate(text.specs):
        assert got.get(i, []) == want.get(i, []), (where, s, got.get(i))
    # and everything equals the oracle's
    assert tuple(r['hits']) == tuple(o['hits']), where
    assert r['hitseqs'] == o['hitseqs'], where
    st, ost = r['stats'], o['stats']
    assert st['readlengths'] == ost['readlengths'] and st['records_parsed'] == ost['records_parsed'], where
    assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], where
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], where


def run(t, text, force=False):
    s = scan.Scanner(t)
    if force:
        s.force_exhaustive(True)
    s.scan_host(text.data)
    r = s.finish()
    info = s.match_info()
    s.close()
    return r, info


@pytest.mark.parametrize('name,bg', TEXTS, ids=lambda v: str(v))
def test_default_route_survivors_are_verified_behind_the_scan_kernel(name, bg):
    """the table without the sequences the seed index refuses: the seed filter and kvq_verify_survivors alone (X: no
    seed index, the exhaustive kernels alone)"""
    w = MM.cell(name)
    text, o = w.texts[bg], oracle_of(name, bg, False)
    t = scan.Table(w.seqs_kept, **w.cfg)
    r, info = run(t, text)
    if name == 'X':
        assert not any(t.seeded) and r['path'] == EXHAUSTIVE_ALONE and r['kernel'] is None, (r['path'], r['kernel'])
        assert info['survivors'] == 0 and info['redo_records'] == 0
    else:
        assert all(t.seeded)
        assert r['path'] == SEEDED_ALONE, r['path']
        assert 0 < info['survivors'] <= info['survivors_cap'] == 1 << 22, info
        assert info['redo_records'] == 0 and info['redo_long'] == 0, info
        if not overridden():
            # maxerrors 4 and 6 (and 1): the draining kernel of 5-base seeds, lanes per tile behind 75-base records (two
            # a read there) and four a read behind 150-base ones, both narrower than maxerrors + 1 (kvq_scan_pick)
            assert (r['kernel']['k'], r['kernel']['dense']) == (w.k, name != 'P'), r['kernel']
            assert r['kernel']['lg'] == (-1 if bg == 75 else 2), r['kernel']
    check(r, o, text, len(w.seqs_kept), (name, bg))
    t.close()


@pytest.mark.parametrize('name', ['P', 'S', 'E4'])
def test_without_a_survivors_list_every_work_item_is_verified_in_place(name, monkeypatch):
    """KVQ_SURV_CAP=0, read when the scan object is made: bp_verify_rest counts every overlap"""
    w = MM.cell(name)
    bg = MM.BACKGROUNDS[name][0]
    text, o = w.texts[bg], oracle_of(name, bg, False)
    monkeypatch.setenv('KVQ_SURV_CAP', '0')
    t = scan.Table(w.seqs_kept, **w.cfg)
    r, info = run(t, text)
    assert r['path'] == SEEDED_ALONE, r['path']
    assert info['survivors_cap'] == 0 and info['survivors'] > 0, info     # (slots asked for, none given)
    check(r, o, text, len(w.seqs_kept), name)
    t.close()


@pytest.mark.parametrize('name,bg', [(n, MM.BACKGROUNDS[n][-1]) for n in MM.CELLS], ids=lambda v: str(v))
def test_forced_exhaustive_route(name, bg):
    """kvq_match_all / within_budget for every record and every sequence"""
    w = MM.cell(name)
    text, o = w.texts[bg], oracle_of(name, bg, True)
    t = scan.Table(w.seqs, **w.cfg)
    r, info = run(t, text, force=True)
    assert r['path'] == EXHAUSTIVE_ALONE and r['kernel'] is None, (r['path'], r['kernel'])
    assert info['survivors'] == 0 and info['redo_records'] == 0, info
    check(r, o, text, len(w.seqs), name)
    t.close()


@pytest.mark.parametrize('name,bg', [(n, MM.BACKGROUNDS[n][0]) for n in MM.CELLS if n != 'X'], ids=lambda v: str(v))
def test_refused_sequences_go_to_the_exhaustive_kernels_beside_the_seed_filter(name, bg):
    """the table with a sequence holding an N, sequences too short for the seed index and one of 4096 bases (one more
    than its 12-bit fields hold), beside the one of 4095"""
    w = MM.cell(name)
    text, o = w.texts[bg], oracle_of(name, bg, True)
    t = scan.Table(w.seqs, **w.cfg)
    assert [i for i, sd in enumerate(t.seeded) if not sd] == w.refused
    r, info = run(t, text)
    assert r['path'] == SEEDED_AND_EXHAUSTIVE, r['path']
    assert 0 < info['survivors'] <= info['survivors_cap'], info
    check(r, o, text, len(w.seqs), name)
    by_seq = {}
    for s in w.specs:
        if s.plan:
            by_seq[s.target] = by_seq.get(s.target, 0) + len(s.plan)
    got = text.by_spec(r['hits'])
    for nr in w.refused + [w.nr[4095]]:
        assert by_seq[nr] > 0 and sum(len(got.get(i, [])) for i, s in enumerate(text.specs) if s.target == nr) == by_seq[nr], nr
    t.close()


# a tile that leaves records behind: only those go through the exhaustive kernels (tests/test_gpu_parity.py)
REDO_PATH = dict(seeded=True, exhaustive=True, rescanned=False, tiles_rescanned=True)


def redo(text, co, expect, seqs=None):
    """a text that leaves records to the redo behind the scan kernel, scanned twice on one scan object (the second time the
    scan object has seen skipped tiles and sizes the redo's launches for that; their grids are not observed here);
    expect(rep, path, match_info)"""
    w = MM.cell('P')
    seqs = w.seqs_kept if seqs is None else seqs
    o = O.scan_memory(text.data, seqs, fold=True, nthreads=16, **w.cfg)
    t = scan.Table(seqs, **w.cfg)
    assert all(t.seeded)
    s = scan.Scanner(t)
    d = scan.DeviceBuffer(text.data.nbytes); d.upload(text.data)
    for rep in range(2):
        s.reset()
        s.scan_device(d.ptr, text.data.nbytes, co)
        r = s.finish()
        expect(rep, r['path'], s.match_info())
        check(r, o, text, len(seqs), rep)
    d.free(); s.close(); t.close()


def test_the_redo_route_matches_short_and_long_reads_of_skipped_tiles():
    """kvq_match_all on the short spec records of skipped tiles, hits and their twins; kvq_match_long on reads of 1024 bases
    and more: every overlap length at the read's head and tail, sequences inside, at every byte shift of the staged read,
    the eight-base prefilter, reads on both sides of the LDS buffer's bound"""
    text, co = MM.long_text()

    def expect(rep, path, info):
        assert path == REDO_PATH, (rep, path)
        # both lists of the redo were used: every record the skipped tiles left (kvq_match_all), the long reads among them (kvq_match_long)
        assert info['redo_records'] == text.n_left and info['redo_long'] == text.n_long <= MM.KVQ_LONG_CAP, (rep, info, text.n_left, text.n_long)
    redo(text, co, expect)


def test_one_long_read_more_than_their_list_holds_is_left_to_the_ordinary_matcher():
    """KVQ_LONG_CAP + 1 reads of 1024 bases in one launch (match_matrix.cap_text): each floods its wave's queue and is put on
    the redo's list of long reads by the scan kernel itself, or is the last record of its tile and comes there through
    kvq_trim_records; both count on one word.  The list takes KVQ_LONG_CAP (kvq_match_long clamps what it reads to that),
    the read that comes when it is full stays an ordinary record of the redo, for kvq_match_all.  The batch is not redone"""
    text, n = MM.cap_text()
    seqs = MM.cell('P').flood_table()

    def expect(rep, path, info):
        if overridden():                # (the draining kernels empty their queues and keep such reads)
            return
        assert path == REDO_PATH, (rep, path)
        assert info['redo_long'] == n == MM.KVQ_LONG_CAP + 1 and 1 <= info['redo_records'] <= MM.KVQ_REDO_RECORDS, (rep, info)
    redo(text, scan.chunk_offsets(text.data), expect, seqs)


def test_tiles_that_leave_more_records_than_the_redo_takes_fail_the_batch():
    """2049 long reads in tiles that overflow their newline tables (match_matrix.overflow_text): more records than the redo's
    list holds, the batch is scanned again as a whole by the exhaustive kernels, where kvq_match_all matches the long reads
    too.  (A scan object that had a batch redone goes back to the tile with the full look-ahead, kvq_scan.hip: the second
    scan has two tiles a chunk, the second of which keeps its records; still more than the list holds)"""
    text, co, n = MM.overflow_text()

    def expect(rep, path, info):
        assert path['rescanned'] is True and path['exhaustive'] is True, (rep, path)
        assert info['redo_records'] > MM.KVQ_REDO_RECORDS and info['redo_long'] == 0, (rep, info)
        assert rep > 0 or info['redo_records'] == text.n_left, (info, text.n_left)
    redo(text, co, expect)
