"""
extract_hits without a GPU: the fallback through Fastq.readrecordat (an analyser whose hits were given, e.g. rebuilt from
JSON) and the formatting of a record as the reference's readrecordat returns it (each line stripped, joined by newlines).
"""
import os

import pytest

from kvarq_amd import analyse, engine
from kvarq_amd.fastq import Fastq


def _analyser_with_hits(path, file_positions):
    a = analyse.Analyser()
    a.fastq = Fastq(path, variant='Sanger', quiet=True)
    a.hits = [engine.Hit(0, fp, 0, 10, 50) for fp in file_positions]
    return a


def test_extract_hits_falls_back_to_readrecordat(tmp_path):
    recs = [b'@r%d some text\n%s\n+\n%s\n' % (i, b'ACGT' * 10 + b'ACG'[:i % 3], b'I' * (40 + i % 3)) for i in range(6)]
    p = tmp_path / 'x.fastq'; p.write_bytes(b''.join(recs))
    starts = [sum(len(r) for r in recs[:i]) for i in range(6)]
    bases = [s + recs[i].index(b'\n') + 1 for i, s in enumerate(starts)]
    # hits in records 3, 1, 3 (a duplicate) and 5, one of them deep inside its read
    a = _analyser_with_hits(str(p), [bases[3], bases[1] + 7, bases[3], bases[5] + 30])
    assert a.records is None
    out = tmp_path / 'hits.fastq'
    a.extract_hits(str(out))
    want = b''.join(recs[i] for i in (3, 1, 3, 5))
    assert out.read_bytes() == want


def test_extract_hits_uses_kept_records_in_hit_order(tmp_path):
    p = tmp_path / 'y.fastq'; p.write_bytes(b'@a\nACGT\n+\nIIII\n')
    a = _analyser_with_hits(str(p), [3, 3])
    a.records = [b'@one \r\nAC GT\t\r\n+\r\n IIII\r\n', '@two\nACGT\n+\nIIII']
    out = tmp_path / 'kept.fastq'
    a.extract_hits(str(out))
    assert out.read_bytes() == b'@one\nAC GT\n+\nIIII\n@two\nACGT\n+\nIIII\n'


@pytest.mark.parametrize('raw, want', [
    (b'@id\nACGT\n+\nIIII\n', b'@id\nACGT\n+\nIIII\n'),
    (b'  @id x  \r\n ACGT\r\n+id \r\n\tIIII \r\n', b'@id x\nACGT\n+id\nIIII\n'),
    (b'@id\nACGT\n+\nIIII', b'@id\nACGT\n+\nIIII\n'),                       # no final newline
    (b'@id\nACGT\n+\nII\x0bII\x0c\r', b'@id\nACGT\n+\nII\x0bII\n'),           # ASCII whitespace only, inner bytes kept
    (b'@id\xa0\nAC\n+\nII\n', b'@id\xa0\nAC\n+\nII\n'),                      # not ASCII whitespace: kept
    (b'@id\nACGT\n', b'@id\nACGT\n\n\n'),                                   # cut short: empty lines, as readline at EOF
])
def test_format_record_strips_each_line(raw, want):
    assert analyse.format_record(raw) == want
    assert analyse.format_record(raw.decode('latin-1')) == want
