"""
The quality trim of every device path, observed per read: texts in which every record hits whatever its trim
(tests/trim_matrix.py; checked without a GPU in tests/test_trim_host.py), so that the (file_pos, readlength) of the
hits are the trim's (start, length) of every record the length gate lets through.  "Observed" means: the set of
these pairs equals the one a plain Python statement of workhorse.c:1055-1068 predicts, besides everything equalling
the oracle's.  The scan kernel's lane split (every lane group, closed form / walk / descent, one round and several),
kvq_trim_records (whole batches on the exhaustive route, the records skipped tiles leave) and kvq_long_line_run.
Bit-exact throughout.
"""
import os

import pytest

import trim_matrix as TM
from kvarq_amd import scan
from oracle import oracle as O
from test_gpu_kernel_matrix import OVERRIDES

pytestmark = pytest.mark.gpu

# a tile that leaves records behind: only those go through the exhaustive kernels (tests/test_gpu_parity.py)
REDO_PATH = dict(seeded=True, exhaustive=True, rescanned=False, tiles_rescanned=True)

_oracle = {}


def oracle_of(key, text, seqs):
    """one oracle run per text, shared by the tests that want it"""
    if key not in _oracle:
        _oracle[key] = O.scan_memory(text.data, seqs, fold=True, nthreads=16, **text.cfg)
    return _oracle[key]


def overridden():
    return any(os.environ.get(v) for v in OVERRIDES)


def check(r, o, text, where):
    # every record reveals its trim: the hits carry the (start, length) the plain statement predicts, no other and no less
    want = text.revealed()
    got = set((h.file_pos, h.readlength) for h in r['hits'])
    assert len(want) >= len(text.records) // 4
    assert got == want, (where, sorted(want - got)[:5], sorted(got - want)[:5])
    assert r['stats']['readlengths'] == text.readlengths(), where
    # and everything equals the oracle's
    assert tuple(r['hits']) == tuple(o['hits']), where
    assert r['hitseqs'] == o['hitseqs'], where
    st, ost = r['stats'], o['stats']
    assert st['readlengths'] == ost['readlengths'], where
    assert st['records_parsed'] == ost['records_parsed'] == len(text.records), where
    assert st['nseqhits'] == ost['nseqhits'] and st['nseqbasehits'] == ost['nseqbasehits'], where
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations'], where


def scan_host(t, text, force=False):
    s = scan.Scanner(t)
    if force:
        s.force_exhaustive(True)
    s.scan_host(text.data)
    r = s.finish()
    s.close()
    return r


@pytest.mark.parametrize('cell', TM.CELLS, ids=TM.cell_id)
def test_scan_kernel_trims_every_record_as_the_statement_does(cell):
    lg, dense = cell
    w = TM.workload(lg, dense)
    t = scan.Table(w.seqs, **w.cfg)
    for i, text in enumerate(w.texts):
        o = oracle_of((cell, i), text, w.seqs)
        r = scan_host(t, text)
        if not overridden():
            assert (r['kernel']['lg'], r['kernel']['dense']) == (lg, dense), (i, r['kernel'])
            assert r['path']['seeded'] is True, (i, r['path'])
        check(r, o, text, i)
    t.close()


def test_the_exhaustive_route_trims_every_record_as_the_statement_does():
    """the texts of the four-lane cell through kvq_trim_records: forced, and by a table whose template holds an N
    (refused by the seed index; every read carries the same N, and equal bytes match)"""
    w, wn = TM.workload(2, False), TM.workload(2, False, True)
    t, tn = scan.Table(w.seqs, **w.cfg), scan.Table(wn.seqs, **wn.cfg)
    assert tn.seeded == [False, True, False, True] and t.seeded == [True] * 4
    for i, (text, textn) in enumerate(zip(w.texts, wn.texts)):
        o = oracle_of(((2, False), i), text, w.seqs)
        r = scan_host(t, text, force=True)
        assert r['path']['seeded'] is False and r['path']['exhaustive'] is True, (i, r['path'])
        check(r, o, text, ('forced', i))
        on = oracle_of(('n', i), textn, wn.seqs)
        rn = scan_host(tn, textn)
        assert rn['path']['exhaustive'] is True, (i, rn['path'])
        check(rn, on, textn, ('n', i))
        # the N changes the route and nothing else
        assert tuple(rn['hits']) == tuple(r['hits']) and textn.revealed() == text.revealed()
    t.close(); tn.close()


@pytest.mark.parametrize('k', [8, 5])
def test_the_redo_trims_long_and_left_records_as_the_statement_does(k):
    """long records their tiles cannot hold (kvq_trim_records a wave a record, kvq_long_line_run from 1024 scores on,
    the long reads' matcher from 1024 trimmed bases on) and tiles of records too short for the tiles' tables"""
    text, co = TM.redo_text(k)
    seqs = TM.table()
    o = oracle_of(('redo', k), text, seqs)
    t = scan.Table(seqs, **text.cfg)
    s = scan.Scanner(t)
    d = scan.DeviceBuffer(text.data.nbytes); d.upload(text.data)
    longs = [(r.read_off + tr[0], tr[1]) for r, tr in zip(text.records, text.trims()) if r.long]
    assert len(longs) == len(TM.LONG_RECORDS) and sum(1 for _, ln in longs if ln >= 1024) >= 3
    for rep in range(2):                                           # (the second time the launches for a scan that has seen skipped tiles)
        s.reset()
        s.scan_device(d.ptr, text.data.nbytes, co)
        r = s.finish()
        assert r['path'] == REDO_PATH, (rep, r['path'])
        check(r, o, text, rep)
        got = set((h.file_pos, h.readlength) for h in r['hits'] if h.seq_nr == 1)
        assert got == set(longs), rep
    d.free(); s.close(); t.close()


@pytest.mark.parametrize('amin', TM.AMINS, ids=lambda a: 'amin%02x' % a)
def test_other_amin_on_the_scan_kernel_and_the_exhaustive_route(amin):
    """Amin '!', 'I' and 0x7E: the constant of the scan kernel's byte-parallel compare and what counts as a bad score;
    score bytes Amin - 1, Amin, 0x7F, 0x80 and 0xFF"""
    text = TM.amin_text(amin)
    seqs = TM.table()
    o = oracle_of(('amin', amin), text, seqs)
    t = scan.Table(seqs, **text.cfg)
    r = scan_host(t, text)
    if not overridden():
        assert r['path']['seeded'] is True and r['kernel']['lg'] == 2, (r['path'], r['kernel'])
    check(r, o, text, 'seeded')
    r = scan_host(t, text, force=True)
    assert r['path']['seeded'] is False, r['path']
    check(r, o, text, 'forced')
    t.close()
