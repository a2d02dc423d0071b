"""
The record walk that the three CPU twins share (kvq_twins.cpp: "every four newlines of a chunk are a record"), without a GPU:
``kvq_profile_host``, ``kvq_cycles_host`` and ``kvq_reads_host`` agree with each other on WHICH lines are records -- over chunks
that end in an incomplete record, no chunks, no text, an empty chunk among others -- and each refuses bad arguments by its own name.
"""
import ctypes as C

import numpy as np
import pytest

import cases
from kvarq_amd import _lib, profile as P

REC = [cases.rec('r%d' % i, 'ACGTN'[:1 + i % 5] * (3 + i), 'I5!'[i % 3] * (1 + i % 5) * (3 + i)) for i in range(9)]
ALL = b''.join(REC)
AT = np.cumsum([0] + [len(r) for r in REC]).tolist()


def nth_newline(text, n):
    """the offset behind the n-th newline of text"""
    return [i for i, b in enumerate(text) if b == 10][n - 1] + 1


# name -> (text, chunk offsets, records)
WALKS = {
    'whole records': (ALL, [0, len(ALL)], 9),
    '4k+1 newlines': (ALL, [0, nth_newline(ALL, 4 * 5 + 1)], 5),
    '4k+2 newlines': (ALL, [0, nth_newline(ALL, 4 * 5 + 2)], 5),
    '4k+3 newlines': (ALL, [0, nth_newline(ALL, 4 * 5 + 3)], 5),
    'tails in two chunks': (ALL, [0, nth_newline(ALL, 4 * 2 + 3), AT[3], nth_newline(ALL, 4 * 7 + 2), AT[8], len(ALL)], 2 + 0 + 4 + 0 + 1),
    'no final newline': (ALL[:-1], [0, len(ALL) - 1], 8),
    'zero chunks': (ALL, [0], 0),
    'empty text': (b'', [0, 0], 0),
    'empty chunk in the middle': (ALL, [0, AT[4], AT[4], len(ALL)], 9),
    'only empty chunks': (ALL, [AT[2], AT[2], AT[2]], 0),
}


@pytest.mark.parametrize('name', sorted(WALKS))
def test_the_twins_agree_on_the_records(name):
    text, co, records = WALKS[name]
    p = P.profile_host(text, (), co, cycles=True, per_read=True, duplication=True)
    assert p.records == records
    assert int(p.reads[P.READS_RECORDS]) == records                        # the reads twin
    assert int(p.cycle_scores[0].sum()) == int(p.cycle_bases[0].sum()) == records      # the cycles twin: no line of these texts is empty
    assert p.duplication['keyed'] == records and p.duplication['unkeyed'] == 0


def test_each_twin_refuses_bad_arguments_by_its_own_name():
    L = _lib.lib()
    text = np.frombuffer(ALL, dtype=np.uint8)
    out = np.zeros(max(P.profile_len(0), P.CYCLES_LEN, P.READS_LEN), dtype=np.int64)
    o = out.ctypes.data_as(C.POINTER(C.c_int64))

    def co(*v):
        return (C.c_int64 * len(v))(*v)
    twins = {'kvq_profile_host': lambda nbytes, c, n, dst=o: L.kvq_profile_host(text.ctypes.data, nbytes, c, n, None, 0, dst),
             'kvq_cycles_host': lambda nbytes, c, n, dst=o: L.kvq_cycles_host(text.ctypes.data, nbytes, c, n, dst),
             'kvq_reads_host': lambda nbytes, c, n, dst=o: L.kvq_reads_host(text.ctypes.data, nbytes, c, n, 0, dst, None)}
    bad = [(-1, co(0, 0), 1), (len(ALL), co(0, len(ALL)), -1), (len(ALL), None, 1), (len(ALL), co(0, len(ALL) + 1), 1),
           (len(ALL), co(-1, len(ALL)), 1), (len(ALL), co(0, AT[5], AT[4], len(ALL)), 3)]
    for name, call in twins.items():
        for args in bad:
            assert call(*args) == _lib.ERR_RUNTIME and _lib.last_error() == (_lib.ERR_RUNTIME, name + ': bad arguments'), (name, args)
        assert call(len(ALL), co(0, len(ALL)), 1) == 0 and _lib.last_error()[0] == 0
    # nowhere to write to: the profile and the cycles refuse, the reads twin has nothing to do
    assert twins['kvq_profile_host'](len(ALL), co(0, len(ALL)), 1, None) == _lib.ERR_RUNTIME and 'kvq_profile_host: bad arguments' in _lib.last_error()[1]
    assert twins['kvq_cycles_host'](len(ALL), co(0, len(ALL)), 1, None) == _lib.ERR_RUNTIME and 'kvq_cycles_host: bad arguments' in _lib.last_error()[1]
    assert twins['kvq_reads_host'](len(ALL), co(0, len(ALL)), 1, None) == 0
    # more than eight cutoffs, or cutoffs that are not there
    assert L.kvq_profile_host(text.ctypes.data, len(ALL), co(0, len(ALL)), 1, None, 1, o) == _lib.ERR_RUNTIME
    assert L.kvq_profile_host(text.ctypes.data, len(ALL), co(0, len(ALL)), 1, text.ctypes.data, 9, o) == _lib.ERR_RUNTIME
    assert _lib.last_error()[1] == 'kvq_profile_host: bad arguments'
