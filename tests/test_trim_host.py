"""
CPU-only checks of the texts tests/test_gpu_trim.py runs on the GPU (tests/trim_matrix.py): the plain statement of
the quality trim against known answers, and for every text that the oracle reveals the trim of every record the
length gate lets through -- its hits carry exactly the (file_pos, readlength) pairs the statement predicts, none
missing, none besides -- that the bands of a family hold what the family promises for the lanes of the cell, and that
every named case of the families occurs.
"""
import bisect
import collections
import os

import pytest

import test_kernel_dispatch as KD
import trim_matrix as TM
from kvarq_amd import scan
from oracle import oracle as O

NTHREADS = min(16, os.cpu_count() or 1)


def test_trim_known_answers(fastqs):
    t = TM.trim
    assert t(b'', 46) == (0, 0)
    assert t(b'#', 46) == (0, 0)
    assert t(b'I', 46) == (0, 1)                         # the newline closes the last run
    assert t(b'#I', 46) == (1, 1)
    assert t(b'II#II', 46) == (0, 2)                     # the first of equally long runs
    assert t(b'II#III', 46) == (3, 3)
    assert t(b'I#II#II#', 46) == (2, 2)
    assert t(b'#####', 46) == (0, 0)
    assert t(b'.-.', 46) == (0, 1)                       # Amin itself is good, Amin - 1 is not
    assert t(b'--..-...', 46) == (5, 3)
    assert t(b'\x7f\x7f\x80\xff\x7f\x7f\x7f', 46) == (4, 3)          # signed char: 0x80 .. 0xFF lie below every Amin
    assert t(b'\x7f\x7f\x80\xff\x7f\x7f\x7f', 0x7E) == (4, 3)
    assert t(b'~~~}~~\x7f', 0x7E) == (0, 3) and t(b'~~~}~~\x7f~', 0x7E) == (4, 4)
    assert t(b'II\rIII\t \x01IIII', 46) == (9, 4)
    assert t(b'@III', 46) == (0, 4) and t(b'+III', 46) == (1, 3) and t(b'+III', 33) == (0, 4)
    # the reference's own fixture (test_engine.py:257-271, tests/test_oracle_kat.py::test_Amin)
    lines = open(os.path.join(fastqs, 'test_engine.fastq'), 'rb').read().split(b'\n')
    lengths = [t(q, ord('H'))[1] for q in lines[3::4]]
    assert lengths.count(5) == 3 and lengths.count(4) == 5


def test_slices_and_census_known_answers():
    assert TM.slices(10, 4) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert TM.slices(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]        # an empty slice
    assert TM.slices(1, 8)[1:] == [(1, 1)] * 7
    p = lambda s: [c == 'I' for c in s]
    assert TM.closed_census(p('IIII' 'I###' 'IIII'), 3) == {'c0', 'c3', 'adj2', 'adj3', 'last'}
    assert TM.closed_census(p('#IIII#I#'), 1) == {'c3', 'bit0', 'last', 'gap1'}
    assert TM.closed_census(p('II#II#II' '#I#I#III'), 2) == {'c2', 'c3', 'bit0', 'gap3'}
    assert TM.closed_census(p('III#' '#III'), 2) >= {'straddle', 'bit0', 'last', 'c1'}
    assert TM.closed_census(p('####' 'IIII'), 2) == set()
    assert TM.ties_census(p('#II#II##' '########'), 2) == {'in-slice'}
    assert TM.ties_census(p('#II#####' '#II#####'), 2) == {'diff-slices'}
    assert TM.ties_census(p('#III####' '######II' 'I#######'), 3) == {'cross-later'}
    assert TM.ties_census(p('######II' 'I####III'), 2) == {'cross-first', }
    assert TM.ties_census(p('#II#II#I' 'I#######'), 2) == {'three', 'in-slice', 'cross-later'}
    assert TM.ties_census(p('##II' 'IIII' 'II##'), 3) == {'span3'}
    assert TM.ties_census(p('#I##' '#III'), 2) == {'at-end'}
    assert TM.tiny_census([1], 4) == {'Q=1', 'empty-slice'} and TM.tiny_census([1] * 5, 4) == {'Q=5', 'empty-slice'}
    assert TM.tiny_census([1] * 4, 4) == {'Q=4'}


def check_revealed(text, seqs):
    """the oracle's histogram is the statement's, and its hits reveal every record the length gate lets through"""
    o = O.scan_memory(text.data, seqs, nthreads=NTHREADS, **text.cfg)
    assert o['stats']['records_parsed'] == len(text.records)
    assert o['stats']['readlengths'] == text.readlengths()
    want = text.revealed()
    got = set((h.file_pos, h.readlength) for h in o['hits'])
    assert len(want - got) == 0, ('records the oracle does not reveal', sorted(want - got)[:5])
    assert len(got - want) == 0, ('hits the statement does not predict', sorted(got - want)[:5])
    return o, want


def check_reaches_the_scan_kernel(text):
    """no tile holds more records than its tables do (such a tile would leave its records to the redo)"""
    offs = [r.start for r in text.records]
    limit = TM.TILE_NEWLINES // 4 - 2
    assert all(b - a >= TM.TILE_OWNS + 4160 for a, b in zip(offs, offs[limit:]))


def lanes_of_records(text, tile):
    """the lanes the general kernel gives each record: it picks them per tile from the records the tile owns.  The
    tiles as kvq_seeded_launch lays them over the chunks (kvq_validate_tiles: tile tn of a chunk at a owns
    (a & ~15) + tn * tile onwards); a record is its tile's when the newline in front of it is (the chunk's first: tile 0)"""
    co = scan.chunk_offsets(text.data).tolist()
    where = []
    for r in text.records:
        c = bisect.bisect_right(co, r.start) - 1
        where.append((c, 0 if r.start == co[c] else max(0, (r.start - 1 - (co[c] & ~15)) // tile)))
    count = collections.Counter(where)
    return [TM.lanes_of_a_tile(count[w]) for w in where]


def check_bands(text, at_g):
    seen = set()
    for name, first, last, L in text.bands:
        recs = [r for r, ok in zip(text.records[first:last], at_g[first:last]) if ok]
        assert recs
        if name in ('mixed', 'tail'):
            continue
        seen.add(name)
        assert all(r.family == name for r in recs)
        # a tile that lies wholly inside the band whichever way the tiles fall
        assert text.records[last - 1].start - text.records[first].start >= 2 * TM.TILE_OWNS + 4160
        top = [max(TM.bad_counts(r.pat, text.G)) for r in recs]
        if name == 'clean':
            assert max(top) == 0
        elif name == 'closed':
            assert max(top) <= 3 and top.count(3) * 10 >= len(top)
        elif name == 'walk':
            assert all(4 <= c <= 8 for c in top)
        elif name == 'descent':
            assert all(c > 8 for c in top)
    return seen


def check_census(text, at_g):
    """every named case occurs in a record that runs with the lanes the case is aimed at and counted for"""
    census = dict(closed={}, ties={}, tiny={})
    for r, ok in zip(text.records, at_g):
        if r.family in census and ok:
            # the lanes of the record: the cell's, at the length the text's head gives
            got = dict(closed=TM.closed_census, ties=TM.ties_census, tiny=TM.tiny_census)[r.family](r.pat, text.G)
            for c in got:
                census[r.family][c] = census[r.family].get(c, 0) + 1
    for fam, want in (('closed', TM.closed_cases(text.G)), ('ties', TM.ties_cases(text.G)), ('tiny', TM.tiny_cases(text.G))):
        missing = [c for c in want if not census[fam].get(c)]
        assert not missing, (fam, missing, census[fam])
    return census


@pytest.mark.parametrize('cell', TM.CELLS, ids=TM.cell_id)
def test_every_record_of_a_cell_is_revealed_and_the_bands_hold_their_families(cell):
    lg, dense = cell
    w = TM.workload(lg, dense)
    cfg = w.cfg
    k, e = TM.KM.seed_k(cfg), cfg['maxerrors']
    assert len(w.texts) == 2
    shown = set()
    for i, text in enumerate(w.texts):
        assert text.data.nbytes < 1500000 and len(text.records) >= 500, (i, text.data.nbytes, len(text.records))
        # the text lands on the cell: tile and lane group from its head, seed length and family from table and settings
        tile, rb = KD.tile_for_text(text.data)
        if not os.environ.get('KVQ_TILE'):
            got = KD.pick(k, TM.KM.index_stride(w.seqs, k, e), dense, rb, tile)
            assert got['lg'] == lg and got['dense'] == dense and got['k'] == k, (i, got)
            if lg < 0:
                assert text.G == TM.lanes_of_a_tile(tile // rb + 1), (i, tile, rb)
        # the lanes the cases are aimed at and counted for are the lanes the kernel uses: the cell's, or, where the kernel
        # picks them per tile, those of the tile a record falls in.  Only the short last tile of a chunk has others; its
        # records count for nothing here
        at_g = [True] * len(text.records)
        if lg > 0:
            assert text.G == 1 << lg
        elif not os.environ.get('KVQ_TILE'):
            lanes = lanes_of_records(text, tile)
            at_g = [g == text.G for g in lanes]
            assert sum(at_g) * 100 >= 95 * len(at_g), (i, collections.Counter(lanes))
            for fam in ('closed', 'ties', 'tiny', 'walk', 'descent'):
                ok = [a for r, a in zip(text.records, at_g) if r.family == fam]
                assert sum(ok) * 100 >= 90 * len(ok), (i, fam, sum(ok), len(ok))
        check_reaches_the_scan_kernel(text)
        o, want = check_revealed(text, w.seqs)
        assert len(want) >= len(text.records) // 4
        seen = check_bands(text, at_g)
        if i == 0 or lg < 0:
            assert seen == set(TM.BANDED)
        check_census(text, at_g)
        # the body of other lengths: slices of more than 64 scores (several rounds, and a merge inside a lane)
        if lg > 0 and i == 1:
            assert any(-(-L // text.G) > 64 for _, _, _, L in text.bands)
        for r, (s, ln), ok in zip(text.records, text.trims(), at_g):
            if r.family == 'ties' and ln >= cfg['minreadlength'] and ok:
                shown |= TM.ties_census(r.pat, text.G)
    # every kind of tie is shown by a hit, not by the histogram alone (start and length).  Two equally long runs inside
    # one slice of a 40- or a 600-base read (one and sixteen lanes) are shorter than the product's minreadlength: the
    # general kernel's draining cell shows those
    want = set(c for text in w.texts for c in TM.ties_cases(text.G))
    assert shown >= want - ({'in-slice'} if cell == (-1, False) else set()), shown


def test_the_table_with_an_n_changes_nothing_but_the_route():
    w, wn = TM.workload(2, False), TM.workload(2, False, True)
    e = w.cfg['maxerrors']
    assert TM.KM.seedable(w.seqs[0], 8, e) and not TM.KM.seedable(wn.seqs[0], 8, e) and TM.KM.seedable(wn.seqs[1], 8, e)
    for text, textn in zip(w.texts, wn.texts):
        assert [r.scores for r in text.records] == [r.scores for r in textn.records]
        assert (text.data != textn.data).sum() > 100 and set(textn.data[text.data != textn.data].tolist()) == {ord('N')}
        o, want = check_revealed(text, w.seqs)
        on, wantn = check_revealed(textn, wn.seqs)
        assert want == wantn and tuple(o['hits']) == tuple(on['hits'])


@pytest.mark.parametrize('amin', TM.AMINS)
def test_every_record_of_an_amin_text_is_revealed(amin):
    text = TM.amin_text(amin)
    assert text.data.nbytes < 1500000
    o, want = check_revealed(text, TM.table())
    assert len(want) >= len(text.records) // 4
    used = set(b for r in text.records for b in r.scores)
    assert used >= set(TM.good_bytes(amin)) | set(TM.bad_bytes(amin)) and {amin, (amin - 1) & 255, 0x7F, 0x80, 0xFF} <= used
    assert any(r.scores[:1] == b'@' for r in text.records) == (amin <= ord('@'))
    assert any(r.scores[:1] == b'+' for r in text.records) == (amin <= ord('+'))


@pytest.mark.parametrize('k', [8, 5])
def test_every_record_of_the_redo_text_is_revealed(k):
    text, co = TM.redo_text(k)
    assert text.data.nbytes < 1500000
    o, want = check_revealed(text, TM.table())
    longs = [(r, tr) for r, tr in zip(text.records, text.trims()) if r.long]
    assert sorted(len(r.scores) for r, _ in longs) == sorted(q for q, _ in TM.LONG_RECORDS) and len(longs) >= 20
    assert set(q for q, _ in TM.LONG_RECORDS) == {1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 9000}
    hits = set((h.seq_nr, h.file_pos, h.readlength) for h in o['hits'])
    for (r, (s, ln)), (Q, kind) in zip(longs, TM.LONG_RECORDS):
        assert ln >= 64 and (1, r.read_off + s, ln) in hits, (Q, kind)          # the probe, inside the run the trim picks
        if kind == 'seam16':
            assert s // 16 != (s + ln - 1) // 16 and s % 16 and ln < 200
        elif kind == 'seam1k':
            assert s // 1024 != (s + ln - 1) // 1024 and ln < 200
        elif kind == 'seam4k':
            assert s < 4096 < s + ln and ln < 200
        elif kind == 'flush':
            assert s + ln == Q
        elif kind == 'big':
            assert ln >= 1024
        elif kind == 'ties':
            assert sum(1 for _, n in TM.runs_of(r.pat) if n == ln) == 2
    assert sum(1 for _, (s, ln) in longs if ln >= 1024) >= 3 and sum(1 for _, (s, ln) in longs if ln < 200) >= 3
    # each long record starts inside its chunk's first tile and ends beyond that tile's look-ahead
    starts = co.tolist()
    for r, _ in longs:
        c = max(a for a in starts if a <= r.start)
        at = r.start - c
        assert at < TM.TILE_OWNS - 160 and at + 2 * len(r.scores) + 25 > TM.TILE_OWNS + TM.LOOKAHEAD + 160
    # the stretch of short records: more of them in any tile than its tables hold
    name, first, last, _ = [b for b in text.bands if b[0] == 'short'][0]
    offs = [r.start for r in text.records[first:last]]
    assert offs[-1] - offs[0] >= 2 * TM.TILE_OWNS + 4160
    assert all(b - a < TM.TILE_OWNS - 4160 for a, b in zip(offs, offs[TM.TILE_NEWLINES // 4:]))
    fams = set(r.family for r in text.records[first:last])
    assert fams >= {'ties', 'bytes'}
    assert any(len(TM.ties_census(r.pat, 1) & {'in-slice'}) and tr[1] >= text.cfg['minreadlength']
               for r, tr in zip(text.records[first:last], text.trims()[first:last]) if r.family == 'ties') == (k == 5)
    # the chunk cuts fall on record starts
    rec_starts = set(r.start for r in text.records) | {text.data.nbytes}
    assert all(c in rec_starts for c in starts) and starts[0] == 0 and starts[-1] == text.data.nbytes
