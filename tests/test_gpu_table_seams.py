"""
The seed index at its seams (tests/table_seams.py; checked without a GPU in tests/test_table_seams_host.py): tables of tandem
repeats, of twins and nested sequences, and the two tables that fill the 20-bit fields of an index entry, through every
route that reads the index -- kvq_verify_survivors behind the scan kernel (the default), bp_verify_rest inside it
(KVQ_SURV_CAP=0), kvq_seed_list (the read-list route) -- and through the exhaustive kernels, the third statement.

Every scan equals the oracle's bit for bit (hits in order, hit bytes, nseqhits, nseqbasehits, read lengths, coverage,
mutations), and the hits of every named record on each of its target sequences equal what match_matrix.alignments planned,
so that a failure names the record.  Every route is taken on purpose and asserted (``path``, ``kernel``,
``Scanner.match_info()``): a test whose route was not taken fails.  Each text is fed as one batch and cut in two.
"""
import os

import pytest

import table_seams as TS
from kvarq_amd import scan
from oracle import oracle as O
from test_gpu_kernel_matrix import OVERRIDES, SEEDED_ALONE, SEEDED_AND_EXHAUSTIVE

pytestmark = pytest.mark.gpu

MAKES, make_of = TS.MAKES, TS.make_of

EXHAUSTIVE_ALONE = dict(seeded=False, exhaustive=True, rescanned=False, tiles_rescanned=False)
SMALL = [m for m in MAKES if m[0] in ('R', 'T')]
LIGHT = [m for m in SMALL if m[3] is not True]                       # R-light and T
HEAVY = [m for m in SMALL if m[3] is True]
_oracle = {}


def oracle_of(m):
    """one oracle run per text, shared by the tests of the module"""
    if m not in _oracle:
        w = make_of(*m)
        _oracle[m] = O.scan_memory(w.data, w.seqs, fold=True, nthreads=16, **w.cfg)
    return _oracle[m]


def overridden():
    return any(os.environ.get(v) for v in OVERRIDES)


def check(r, o, w, where):
    # per record and target: the statement's hits, no other and no less
    got, want = w.by_spec(r['hits']), w.planned()
    assert len(want) >= len(w.specs) // 3
    for i, s in enumerate(w.specs):
        for t in s.targets:
            assert got.get((i, t), []) == want.get((i, t), []), (where, s, t, got.get((i, t)))
    # and everything equals the oracle's
    assert tuple(r['hits']) == tuple(o['hits']), where
    assert r['hitseqs'] == o['hitseqs'], where
    st, ost = r['stats'], o['stats']
    assert st['readlengths'] == ost['readlengths'] and st['records_parsed'] == ost['records_parsed'] == len(w.specs), where
    assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], where
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], where


def run(t, w, batches=1, force=False, **options):
    """-> (result, match_info) of the text fed as one batch, or cut in two at a record's first byte"""
    s = scan.Scanner(t, **options)
    if force:
        s.force_exhaustive(True)
    if batches == 1:
        s.scan_host(w.data)
    else:
        s.scan_host(w.data[:w.cut])
        s.scan_host(w.data[w.cut:], fpos_base=w.cut)
    r = s.finish()
    info = s.match_info()
    s.close()
    return r, info


def table_of(w):
    t = scan.Table(w.seqs, **w.cfg)
    assert overridden() or (t.seeded == w.seeded and t.seed_k == w.k)          # (KVQ_K lowers the seed length: the index then takes shorter sequences)
    return t


def kernel_is(r, w):
    """the scan kernel the configuration and the table were built to reach: the halving one for the product's cell, a draining
    one for seeds shorter than 8 (and for the F tables, whatever their density says)"""
    if overridden():
        return
    assert (r['kernel']['k'], r['kernel']['stride']) == (w.k, w.stride), r['kernel']
    if w.fam in ('Rl', 'Rh', 'T'):
        assert r['kernel']['dense'] == (w.k < 8), r['kernel']


@pytest.mark.parametrize('batches', (1, 2))
@pytest.mark.parametrize('m', LIGHT, ids=TS.make_id)
def test_light_reads_and_twins_by_the_default_route(m, batches):
    """kvq_verify_survivors verifies what the scan kernel found; no read floods a queue, nothing is left to a redo"""
    w, o = make_of(*m), oracle_of(m)
    t = table_of(w)
    r, info = run(t, w, batches)
    assert r['path'] == SEEDED_ALONE, r['path']
    assert 0 < info['survivors'] <= info['survivors_cap'] and info['redo_records'] == 0 and info['redo_long'] == 0, info
    kernel_is(r, w)
    check(r, o, w, (m, batches))
    t.close()


@pytest.mark.parametrize('batches', (1, 2))
@pytest.mark.parametrize('m', HEAVY, ids=TS.make_id)
def test_heavy_repeat_reads_by_the_default_route(m, batches):
    """pure repeat reads, hundreds of hits each: the draining kernels keep them all; the halving kernel (the product's cell)
    may leave a read that floods its wave's queue to the redo, which is not asserted either way (the count seen is in
    profiles/table_seam_tests.txt)"""
    w, o = make_of(*m), oracle_of(m)
    t = table_of(w)
    r, info = run(t, w, batches)
    print('%s, %d batch(es): path %s, match_info %s' % (m, batches, r['path'], info))
    assert r['path']['seeded'] and not r['path']['rescanned'], r['path']
    if w.k < 8 and not overridden():
        assert r['path'] == SEEDED_ALONE and info['redo_records'] == 0, (r['path'], info)
    kernel_is(r, w)
    check(r, o, w, (m, batches))
    t.close()


@pytest.mark.parametrize('m', MAKES, ids=TS.make_id)
def test_without_a_survivors_list_bp_verify_rest_verifies_in_place(m, monkeypatch):
    """KVQ_SURV_CAP=0, read when the scan object is made (the F tables too: bp_verify_rest unpacks the entry word itself)"""
    w, o = make_of(*m), oracle_of(m)
    monkeypatch.setenv('KVQ_SURV_CAP', '0')
    t = table_of(w)
    r, info = run(t, w)
    assert r['path']['seeded'] and not r['path']['rescanned'], r['path']
    assert info['survivors_cap'] == 0 and info['survivors'] > 0, info           # (slots asked for, none given)
    if m[3] is not True:
        assert r['path'] == (SEEDED_ALONE if all(w.seeded) else SEEDED_AND_EXHAUSTIVE) and info['redo_records'] == 0, (r['path'], info)
    kernel_is(r, w)
    check(r, o, w, m)
    t.close()


@pytest.mark.parametrize('m', MAKES, ids=TS.make_id)
def test_the_read_list_route_over_the_same_index(m):
    """Scanner(long_reads=True): kvq_seed_list unpacks the entries and states the canonical discoverer for itself"""
    w, o = make_of(*m), oracle_of(m)
    t = table_of(w)
    r, info = run(t, w, long_reads=True)
    assert r['path']['read_list'] and not r['path']['seeded'] and not r['path']['rescanned'], r['path']
    assert r['path']['exhaustive'] == (not all(w.seeded)), r['path']
    check(r, o, w, m)
    t.close()


@pytest.mark.parametrize('m', MAKES, ids=TS.make_id)
def test_the_forced_exhaustive_route(m):
    """kvq_match_all on every record and every sequence: the statement that knows no index"""
    w, o = make_of(*m), oracle_of(m)
    t = table_of(w)
    r, info = run(t, w, force=True)
    assert r['path'] == EXHAUSTIVE_ALONE and r['kernel'] is None, (r['path'], r['kernel'])
    assert info['survivors'] == 0 and info['redo_records'] == 0, info
    check(r, o, w, m)
    t.close()


@pytest.mark.parametrize('batches', (1, 2))
@pytest.mark.parametrize('fam', ('Fo', 'Fn'))
def test_the_tables_that_fill_the_20_bit_fields(fam, batches):
    """F-offset: a seeded sequence across table offset 2^20, the next ones refused for their offset alone, entry numbers
    above 2^20.  F-number: sequence numbers up to 87 381 in the index, 87 382 and beyond refused.  The seed filter and the
    exhaustive kernels side by side"""
    m = (fam, None, None, None)
    w, o = make_of(*m), oracle_of(m)
    t = table_of(w)
    off = [t.seq_offset[i] for i in range(len(w.seqs) + 1)]
    assert off == TS.offsets_of(w.seqs)
    if fam == 'Fo':
        assert t.seeded == [True] * 258 + [False] * 3 and off[257] == (1 << 20) - 1 and off[258] == (1 << 20) + 59
    else:
        assert t.seeded == [True] * 87382 + [False] * 118 and off[87381] == 1048572 and off[87382] == 1048584
    r, info = run(t, w, batches)
    assert r['path'] == SEEDED_AND_EXHAUSTIVE, r['path']
    assert 0 < info['survivors'] <= info['survivors_cap'] and info['redo_records'] == 0, info
    kernel_is(r, w)
    check(r, o, w, (fam, batches))
    # the named sequences were hit, the refused ones among them
    hit = set(h.seq_nr for h in r['hits'])
    assert hit >= ({0, 128, 255, 256, 257, 258, 259} if fam == 'Fo' else set(TS.FNumber.PLANTED)), sorted(hit)[:20]
    t.close()
