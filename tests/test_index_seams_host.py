"""
The seam matrix of the record index without a GPU (tests/index_seams.py): the statement of the exact
index against a second, independent one and against the host twins, every case against the seams it names, and every wrong
statement -- the right one with one plausible kernel slip -- against the cases, so that the matrix
tests/test_gpu_index_seams.py holds the kernels to is known to tell such a slip.
"""
import numpy as np
import pytest

import index_seams as S
import profile_ref as R
from kvarq_amd import profile as P

INDEX_CASES = S.index_cases()
SKIP_CASES = S.skip_cases()
ids = lambda c: c.name      # noqa: E731


def check_statements(c):
    ix = S.index_of(c.text, c.co)
    per, nl4 = S.index_numpy(c.text, c.co)
    assert np.array_equal(ix.per, per) and np.array_equal(ix.nl4, nl4), c.name
    assert S.same_index(S.index_shaped(c.text, c.co), ix), c.name
    # rec_start, said once more: the byte behind the last newline of the chunk in front of the record, or the chunk's begin
    a = np.asarray(c.co)[np.searchsorted(np.asarray(c.co), ix.nl4[:, 0], side='right') - 1] if len(ix.nl4) else np.zeros(0)
    for g in range(0, len(ix.rec_start), max(1, len(ix.rec_start) // 500)):
        rs, n0 = int(ix.rec_start[g]), int(ix.nl4[g, 0])
        inside = np.flatnonzero(c.text[int(a[g]):n0] == S.NL)
        assert len(inside) % 4 == 0 and rs == (int(a[g]) + int(inside[-1]) + 1 if len(inside) else int(a[g])), (c.name, g)


@pytest.mark.parametrize('c', INDEX_CASES, ids=ids)
def test_statement_against_statement(c):
    check_statements(c)


def test_statement_against_statement_on_the_random_texts():
    for c in S.random_cases(0):
        check_statements(c)


WELL_FORMED = [S.dense_region(0), S.dense_region(7), S.dense_to_the_end(1, False), S.dense_to_the_end(15, True), S.dense_first_tile(1)] + \
    [S.long_interior(v) for v in S.LONG_VARIANTS]


@pytest.mark.parametrize('sc', SKIP_CASES, ids=ids)
def test_the_host_twin_counts_the_records_of_the_statement(sc):
    ix = S.index_of(sc.data, sc.co)
    twin = P.profile_host(sc.data, [ord('.')], sc.co)
    assert twin.records == len(ix.rec_start) == int(ix.per.sum()) > 0
    assert int(twin.words[R.BASE_LINE_BYTES]) == int((ix.nl4[:, 1] - ix.nl4[:, 0] - 1).sum())


def test_the_host_twin_on_the_text_of_the_routes():
    text, co = S.routes_text()
    ix = S.index_of(text.data, co)
    inside = [r for r in text.records if co[0] <= r.start < co[-1]]
    assert P.profile_host(text.data, [ord('.')], co).records == len(ix.rec_start) == len(inside)
    assert [int(x) for x in ix.rec_start] == [r.start for r in inside]
    assert len(inside) < len(text.records) and co[0] > 0 and co[-1] < text.data.nbytes


@pytest.mark.parametrize('c', INDEX_CASES, ids=ids)
def test_every_case_reaches_the_seams_it_names(c):
    reached = S.seams_of(c.text, c.co)
    assert c.seams and not [s for s in c.seams if s not in reached]
    assert len(c.text) <= 1300000


def test_the_random_texts_are_what_the_issue_asks_for():
    rnd = S.random_cases(0)
    assert len(rnd) == 200 and max(len(c.text) for c in rnd) <= 20 << 10
    dens = [float((c.text == S.NL).mean()) for c in rnd if len(c.text) > 4000]
    assert min(dens) < 1 / 300 and max(dens) > 1 / 2.5
    assert sum(any(a == b for a, b in zip(c.co, c.co[1:])) for c in rnd) > 50
    assert sum(c.co[0] > 0 for c in rnd) > 50 and sum(c.co[-1] < len(c.text) for c in rnd) > 50


@pytest.mark.parametrize('slip', list(S.WRONG))
def test_a_wrong_statement_of_the_index_is_told_by_a_case(slip):
    assert any(not S.same_index(S.WRONG[slip](c.text, c.co), S.index_of(c.text, c.co)) for c in INDEX_CASES), slip


# ---- the statement of the skipped tiles ---------------------------------------------------------------------------------

@pytest.mark.parametrize('sc', WELL_FORMED, ids=ids)
def test_the_tiles_of_a_chunk_share_out_its_records(sc):
    """every tile taken as skipped whole: what the statement gives the tiles is every record of the chunks, each once"""
    tile = S.default_tile(sc.data)
    ix = S.index_of(sc.data, sc.co)
    want = set((int(rs),) + tuple(int(x) for x in n4) for rs, n4 in zip(ix.rec_start, ix.nl4))
    got = [S.skipped_of(sc.data, t._replace(seen=S.seen_of(sc.data, t))) for t in S.tiles_of(sc.co, tile)]
    assert sum(len(g) for g in got) == len(want) and set().union(*got) == want
    # a partial tile leaves the records of its tile from the first one it left on
    for t in S.hypothetical_tiles(sc, tile):
        if S.is_partial(sc.data, sc.co, t):
            whole = S.skipped_of(sc.data, S.without_z(sc.data, sc.co, tile, t))
            assert S.skipped_of(sc.data, t) == set(r for r in whole if r[0] >= t.a) and S.seen_of(sc.data, t) == 0


def test_the_sweep_of_the_dense_region_reaches_the_seams_of_the_walk():
    """on the tiles as the geometry gives them (the GPU test asks the same of the descriptors the scan reports)"""
    reached = set()
    for shift in range(20):
        sc = S.dense_region(shift)
        for t in S.hypothetical_tiles(sc, S.default_tile(sc.data))[1:-1]:
            reached |= S.skip_seams(sc.data, t)
    assert not [s for s in S.DENSE_REGION_SEAMS if s not in reached]


def test_the_other_skipped_cases_reach_theirs():
    ends = [S.dense_to_the_end(m, False) for m in range(1, 16)]
    assert sorted(sc.co[-1] % 16 for sc in ends) == list(range(1, 16))
    for sc in ends + [S.dense_to_the_end(8, True)]:
        tiles = S.hypothetical_tiles(sc, S.default_tile(sc.data))
        last = [t for t in tiles if t.b == sc.co[-1]][-1]
        assert 'b not a multiple of 16' in S.skip_seams(sc.data, last)
        cut = sc.data[sc.co[-1] - 1] != S.NL
        assert cut == sc.name.endswith('cut]') == (sc.oracle_bytes < sc.data.nbytes)
        assert last.own_end - last.own_begin > 15000 and ('a record runs to b' in S.skip_seams(sc.data, last)) == (not cut)
    assert sorted(S.dense_first_tile(m).co[1] % 16 for m in (0, 1, 15)) == [0, 1, 15]
    for v in S.LONG_VARIANTS:
        sc = S.long_interior(v)
        tile = S.default_tile(sc.data)
        part = [t for t in S.hypothetical_tiles(sc, tile) if S.is_partial(sc.data, sc.co, t)]
        assert len(part) == (1 if v in ('last 16 owned bytes', 'to the end') else 2)
        for t in part:
            tn = (t.a - (sc.co[1] & ~15)) // tile
            assert tn >= 1, (v, t)
        if v == 'last 16 owned bytes':
            assert 0 < part[0].own_end - part[0].a <= 16
        if v == 'to the end':
            assert len(S.skipped_of(sc.data, part[0])) == 1 and 'a record runs to b' in S.skip_seams(sc.data, part[0])
        if v == 'two in a row':
            assert part[1].a == max(r[4] for r in S.skipped_of(sc.data, part[0]) if r[0] == part[0].a) + 1


@pytest.mark.parametrize('slip', list(S.WRONG_SKIPPED))
def test_a_wrong_statement_of_the_skipped_tiles_is_told_by_a_case(slip):
    for sc in SKIP_CASES[:4] + SKIP_CASES[20:24] + SKIP_CASES[-4:]:
        tile = S.default_tile(sc.data)
        if any(S.WRONG_SKIPPED[slip](sc, tile, t) != S.skipped_of(sc.data, t) for t in S.hypothetical_tiles(sc, tile)):
            return
    raise AssertionError('no case tells the slip "%s"' % slip)


def test_the_committed_census_names_every_case_and_every_wrong_statement():
    import os
    with open(os.path.join(S.ROOT, 'profiles', 'index_seam_tests.txt')) as f:
        text = f.read()
    for c in INDEX_CASES:
        assert c.name in text, c.name
    for slip in list(S.WRONG) + list(S.WRONG_SKIPPED):
        assert slip in text, slip
    assert 'MISSING' not in text and 'NONE' not in text
