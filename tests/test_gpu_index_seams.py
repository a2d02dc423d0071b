"""
The record index on an MI355X, pinned at its seams (tests/index_seams.py).  The exact index --
kvq_count_lines, kvq_scan_segments, kvq_index_records as run_batch drives them -- observed word for word through
``kvq_scan_index_device`` and held against the plain statement on every index case; the same index through the routes that
feed on it; and kvq_collect_skipped observed through the descriptors kvq_validate_tiles wrote and the entries it left on the
redo list, held against the statement of what a skipped tile must leave.  Every comparison is exact.
"""
import functools

import numpy as np
import pytest

import clip_ref as CR
import index_seams as S
import profile_ref as R
import trim_matrix as TM
from kvarq_amd import profile as P, scan
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REDO_PATH = dict(seeded=True, exhaustive=True, rescanned=False, tiles_rescanned=True)
ids = lambda c: c.name      # noqa: E731


@pytest.fixture(scope='module')
def handle():
    """one scan handle for every index case: its buffers are reused from case to case, and ``ensure`` does not clear them"""
    t = scan.Table(TM.table(), **S.routes_text()[0].cfg)
    s = scan.Scanner(t)
    yield s
    s.close(); t.close()


def upload(text):
    """the text in a buffer whose size is rounded up to 16, newlines behind the text"""
    n = len(text)
    d = scan.DeviceBuffer((n + 15) // 16 * 16)
    d.upload(np.concatenate([np.asarray(text, dtype=np.uint8), np.full((-n) % 16, S.NL, dtype=np.uint8)]))
    return d


def check_index(s, c):
    want = S.index_of(c.text, c.co)
    d = upload(c.text)
    R_, per, nl4, rs = s.index_device(d.ptr, len(c.text), c.co)
    d.free()
    assert R_ == len(want.rec_start), (c.name, R_, len(want.rec_start))
    bad = np.flatnonzero(per != want.per)
    assert bad.size == 0, (c.name, 'records per chunk', bad[:5], per[bad[:5]], want.per[bad[:5]])
    bad = np.flatnonzero((nl4 != want.nl4).any(axis=1))
    assert bad.size == 0, (c.name, 'nl4', bad[:5], nl4[bad[:5]].tolist(), want.nl4[bad[:5]].tolist())
    bad = np.flatnonzero(rs != want.rec_start)
    assert bad.size == 0, (c.name, 'rec_start', bad[:5], rs[bad[:5]], want.rec_start[bad[:5]])


@pytest.mark.parametrize('c', S.index_cases(), ids=ids)
def test_the_index_exactly(handle, c):
    assert c.seams
    check_index(handle, c)
    if len(c.text) > 500000:
        # a small case behind a large one, on the same handle: what the large one left in the buffers must not show
        check_index(handle, S.empty_and_tiny())
        check_index(handle, S.limit())


def test_the_index_exactly_on_the_random_texts(handle):
    check_index(handle, S.segments(300))
    for c in S.random_cases(0):
        check_index(handle, c)


def test_the_index_call_leaves_nothing_behind_and_is_refused_on_a_fed_scan(handle):
    text, co = S.routes_text()
    s = handle
    s.reset()
    d = upload(text.data)
    want = S.index_of(text.data, co)
    assert s.index_device(d.ptr, text.data.nbytes, co)[0] == len(want.rec_start)
    r = s.finish()                                      # nothing was scanned
    assert r['n_hits'] == 0 and r['stats']['records_parsed'] == 0 and r['main_kernel_launches'] == 0
    s.reset()
    R_, per, nl4, rs = s.index_device(d.ptr, text.data.nbytes, co, cap=7)      # a capacity below R: R all the same, seven entries
    assert R_ == len(want.rec_start) and len(rs) == 7 and (nl4 == want.nl4[:7]).all() and (per == want.per).all()
    s.scan_device(d.ptr, text.data.nbytes, co)
    with pytest.raises(Exception):
        s.index_device(d.ptr, text.data.nbytes, co)
    with pytest.raises(Exception):
        s.keep_skipped()
    s.finish()
    with pytest.raises(Exception):
        s.skipped_tiles()                               # (never asked to keep them)
    s.reset()
    with pytest.raises(Exception):
        s.index_device(d.ptr, text.data.nbytes, [0, 10, 5])
    d.free()


# ---- the routes that feed on the index ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def routes_oracle(clip):
    text, co = S.routes_text()
    data = P.clip_host(text.data, CR.PROBES[2], co)[0] if clip else text.data
    return O.scan_memory(data[co[0]:co[-1]], TM.table(), fpos_base=co[0], fold=True, nthreads=16, **text.cfg)


def same_as_oracle(r, o, where):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs'], where
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], (where, k)
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], where


ROUTES = ('exhaustive', 'seeded+profile', 'clip', 'long_reads')


@pytest.mark.parametrize('feed', ['host', 'device'])
@pytest.mark.parametrize('route', ROUTES)
def test_the_routes_on_cuts_of_every_alignment(route, feed):
    text, co = S.routes_text()
    inside = [(r, tr) for r, tr in zip(text.records, text.trims()) if co[0] <= r.start < co[-1]]
    o = routes_oracle(route == 'clip')
    assert o['stats']['records_parsed'] == len(inside)
    kw = {'seeded+profile': dict(profile=[ord('.'), ord('I')]), 'clip': dict(clip=CR.PROBES[2]), 'long_reads': dict(long_reads=True)}.get(route, {})
    t = scan.Table(TM.table(), **text.cfg)
    s = scan.Scanner(t, **kw)
    if route == 'exhaustive':
        s.force_exhaustive(True)
    d = None
    if feed == 'host':
        s.scan_host(text.data, chunk_off=co)
    else:
        d = upload(text.data)
        s.scan_device(d.ptr, text.data.nbytes, co)
    r = s.finish()
    same_as_oracle(r, o, (route, feed))
    if route != 'clip':
        # every record of the chunks reveals itself, and none outside them
        mrl = text.cfg['minreadlength']
        want = set((rec.read_off + st, ln) for rec, (st, ln) in inside if ln >= mrl)
        assert len(want) > len(inside) // 2 and set((h.file_pos, h.readlength) for h in r['hits']) == want
    if route == 'exhaustive':
        assert r['path']['seeded'] is False and r['path']['exhaustive'] is True
    elif route == 'long_reads':
        assert r['path']['read_list'] is True and r['path']['seeded'] is False
    else:
        assert r['path']['seeded'] is True
    if route == 'seeded+profile':
        want = R.profile(text.data.tobytes(), [ord('.'), ord('I')], co)
        assert (r['profile'].words == want).all()
        assert r['profile'].records == len(inside) and int(want[R.BASE_LINE_BYTES]) == int(r['profile'].words[R.BASE_LINE_BYTES])
    if d is not None:
        d.free()
    s.close(); t.close()


# ---- the skipped tiles ---------------------------------------------------------------------------------------------------

def scan_skipped(sc, profile):
    """one scan_device of the case, twice on one handle (the second on a reset handle); -> the first result and its
    descriptors, each checked against the statement"""
    o = O.scan_memory(sc.data[:sc.oracle_bytes], TM.table(), fold=True, nthreads=16, **sc.cfg)
    t = scan.Table(TM.table(), **sc.cfg)
    s = scan.Scanner(t, profile=[ord('.')] if profile else None)
    s.keep_skipped()
    d = upload(sc.data)
    ix = S.index_of(sc.data, sc.co)
    every = set((int(rs),) + tuple(int(x) for x in n4) for rs, n4 in zip(ix.rec_start, ix.nl4))
    out = None
    for rep in range(2):
        s.reset()
        s.scan_device(d.ptr, sc.data.nbytes, sc.co)
        r = s.finish()
        where = (sc.name, rep)
        assert r['path'] == REDO_PATH, (where, r['path'])
        tiles, (nl4, rs) = s.skipped_tiles(), s.redo_list()
        assert len(tiles) > 0, where
        got = [(int(a),) + tuple(int(x) for x in n4) for a, n4 in zip(rs, nl4)]
        want = set()
        for tl in tiles:
            tl = S.Tile(*[int(x) for x in tl])
            assert tl.seen == S.seen_of(sc.data, tl), (where, tl)
            mine = S.skipped_of(sc.data, tl)
            assert not (mine & want), (where, tl, 'two descriptors own a record')
            want |= mine
        assert len(got) == len(set(got)), (where, 'an entry twice')
        assert set(got) == want, (where, sorted(want - set(got))[:4], sorted(set(got) - want)[:4])
        assert want <= every
        assert len(got) == s.match_info()['redo_records'], where
        same_as_oracle(r, o, where)
        assert r['stats']['records_parsed'] == len(ix.rec_start), where
        if profile:
            assert (r['profile'].words == R.profile(sc.data.tobytes(), [ord('.')], sc.co)).all(), where
        if out is None:
            out = (r, [S.Tile(*[int(x) for x in tl]) for tl in tiles])
        else:
            assert tuple(r['hits']) == tuple(out[0]['hits']) and len(tiles) == len(out[1]), where
    d.free(); s.close(); t.close()
    return out


def test_dense_region_sweep():
    """the stretch of short records moved byte by byte: between them the reported descriptors must show every seam of the
    walk (a seam that is missing is the generator's to reach: the assertion names it)"""
    reached, whole = set(), []
    for shift in range(20):
        sc = S.dense_region(shift)
        r, tiles = scan_skipped(sc, profile=shift % 5 == 0)
        interior = [tl for tl in tiles if not tl.first]
        assert 2 <= len(interior) <= 4, (shift, tiles)
        # ... in a row
        assert all(y.own_begin == x.own_end for x, y in zip(sorted(interior), sorted(interior)[1:])), (shift, interior)
        whole.append(len(interior))
        for tl in interior:
            reached |= S.skip_seams(sc.data, tl)
    missing = [s for s in S.DENSE_REGION_SEAMS if s not in reached]
    assert not missing, ('the sweep does not reach', missing, whole)


@pytest.mark.parametrize('sc', [S.dense_to_the_end(m, False) for m in range(1, 16)] + [S.dense_to_the_end(m, True) for m in (1, 8, 15)], ids=ids)
def test_dense_to_the_end(sc):
    r, tiles = scan_skipped(sc, profile=sc.co[-1] % 16 == 8)
    last = [tl for tl in tiles if tl.b == sc.co[-1] and tl.own_end == tl.b]
    assert len(last) == 1 and S.skip_seams(sc.data, last[0]) >= {'b not a multiple of 16'}, tiles
    assert ('a record runs to b' in S.skip_seams(sc.data, last[0])) == (not sc.name.endswith('cut]'))


@pytest.mark.parametrize('sc', [S.dense_first_tile(m) for m in (0, 1, 15)], ids=ids)
def test_dense_first_tile(sc):
    r, tiles = scan_skipped(sc, profile=False)
    first = [tl for tl in tiles if tl.first and tl.a == sc.co[1]]
    assert len(first) == 1 and first[0].own_begin == sc.co[1] and first[0].seen == 0, tiles


@pytest.mark.parametrize('sc', [S.long_interior(v) for v in S.LONG_VARIANTS], ids=ids)
def test_long_interior(sc):
    r, tiles = scan_skipped(sc, profile=True)
    part = [tl for tl in tiles if S.is_partial(sc.data, sc.co, tl)]
    assert part, tiles
    tile = S.default_tile(sc.data)
    for tl in part:
        assert tl.a == tl.own_begin and tl.seen == 0 and (tl.a - (sc.co[1] & ~15)) // tile >= 1, tl
        assert sc.data[tl.a] == ord('@') and sc.data[tl.a - 1] == S.NL
    if 'last 16' in sc.name:
        assert any(0 < tl.own_end - tl.a <= 16 for tl in part), part
    if 'to the end' in sc.name:
        assert any('a record runs to b' in S.skip_seams(sc.data, tl) for tl in part)
    # the long records are matched: the probe is found in each
    longs = [(rec.read_off + tr[0], tr[1]) for rec, tr in zip(sc.text.records, sc.text.trims()) if rec.long]
    assert longs and set((h.file_pos, h.readlength) for h in r['hits'] if h.seq_nr == 1) >= set(longs)

