"""
Every probe count on an MI355X: the adapter content and the adapter clip with n = 1 .. 8 probes, exact and at one mismatch per ten
bases -- the 32 instantiations the launcher picks by n and by the rule (include/kvarq_hip.h, DESIGN sections 18 to 20).  The probes
are ``adapt_ref.EIGHT[:n]`` and ONLY THE LAST OF THE n OCCURS in the text: a kernel for fewer probes finds nothing, and one for
more reads entries that are zero and must find nothing there.  The whole adapters array against the plain statements
(tests/adapt_ref.py, tests/adapt_mm_ref.py), and what the clip leaves in the buffer byte for byte, with its eight words, against
theirs (tests/clip_ref.py, tests/adapt_mm_ref.py).  What the text must be for that is asserted first, from the statements alone.
"""
import functools

import numpy as np
import pytest

import adapt_mm_ref as M
import adapt_ref as A
import clip_ref as CR
from kvarq_amd import scan
from test_gpu_clip import check_clip, scan_device

pytestmark = pytest.mark.gpu

SEQ = [b'ACGTACGTACGTACGTACGTACGTA']
SEED = 1        # (chosen so that the condition on the text holds for every n and both rules: condition() asserts it)
PERS = (None, 10)


@functools.lru_cache(maxsize=None)
def text_of(n):
    """a dozen records over A C G T in which probe n - 1 is planted -- whole in the first round of 224 positions, whole beyond it, as
    a tail only, at the line's start, as the whole line, behind a '\\r' line end -- and no other probe is"""
    rng = np.random.RandomState(SEED + n)
    probe = A.EIGHT[n - 1]

    def fill(k):
        return rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), k).tobytes() if k else b''
    recs = [A.rec(fill(10 + n) + probe + fill(30)),                                  # whole, first round
            A.rec(fill(290 + n) + probe + fill(20)),                                 # whole, second round
            A.rec(fill(60) + probe[:7]),                                             # a tail only
            A.rec(fill(80)),                                                         # none
            A.rec(fill(40) + probe + fill(9), nl=b'\r\n'),                           # whole, the line ends in '\r'
            A.rec(fill(33) + probe[:len(probe) - 1], nl=b'\r\n'),                    # the longest tail, the line ends in '\r'
            A.rec(probe + fill(17)),                                                 # at the line's start
            A.rec(probe),                                                            # the whole line
            A.rec(b''), A.rec(fill(5)),                                              # lines shorter than any tail
            A.rec(fill(230)),                                                        # none, two rounds
            A.rec(fill(150) + probe[:6] + fill(1))]                                  # a tail that the line's last base spoils
    return b''.join(recs)


@functools.lru_cache(maxsize=None)
def statement(n, per):
    """(the adapters array, MASK(text), the clip's eight words) of the plain statements; computed once, left unchanged"""
    text, probes, co = text_of(n), A.EIGHT[:n], [0, len(text_of(n))]
    if per:
        w, (masked, c) = M.adapt(text, co, probes, per), M.mask(text, co, probes, per)
    else:
        w, (masked, c) = A.adapt(text, co, probes), CR.mask(text, co, probes)
    masked = np.frombuffer(masked, dtype=np.uint8)
    for a in (w, c):
        a.flags.writeable = False
    return w, masked, c


def condition(n, per):
    """only the last probe occurs, whole and as a tail; and the records reach what they are built for"""
    w = statement(n, per)[0]
    for k in range(A.MAX_PROBES):
        blk = w[A.BLOCKS + k * A.BLOCK_WORDS:A.BLOCKS + (k + 1) * A.BLOCK_WORDS]
        if k == n - 1:
            assert blk[A.B_FIRST] > 0 and blk[A.B_TAIL] > 0, (n, per, k)
        else:
            assert blk[A.B_FIRST] == 0 and blk[A.B_TAIL] == 0, (n, per, k)
    text, co = text_of(n), [0, len(text_of(n))]
    recs = M.per_record(text, co, A.EIGHT[:n], per) if per else A.per_record(text, co, A.EIGHT[:n])
    first = [r[2][n - 1] for r in recs]
    tail = [r[3][n - 1] for r in recs]
    assert any(f is not None and f < 224 for f in first) and any(f is not None and f >= 224 for f in first) and 0 in first
    assert 7 in tail and len(A.EIGHT[n - 1]) - 1 in tail
    assert any(f is None and t is None and r[1] > 224 for f, t, r in zip(first, tail, recs))
    assert any(r[5] and f is not None for f, r in zip(first, recs)) and any(r[5] and t is not None for t, r in zip(tail, recs))
    assert len(recs) == 12 and len(text) < 4096


@pytest.mark.parametrize('what', ['adapters', 'clip'])
@pytest.mark.parametrize('per', PERS)
@pytest.mark.parametrize('n', range(1, A.MAX_PROBES + 1))
def test_every_probe_count(n, per, what):
    condition(n, per)
    probes = A.EIGHT[:n]
    w, masked, c = statement(n, per)
    arr = np.frombuffer(text_of(n), dtype=np.uint8)
    t = scan.Table(SEQ, **CR.CFG)
    if what == 'adapters':
        r, after = scan_device(t, arr, (0, arr.nbytes), profile=(), adapters=probes, adapter_mismatches=per)
        got = r['profile'].adapters.words
        bad = np.nonzero(got != w)[0]
        assert bad.size == 0, (bad[:8], got[bad[:8]], w[bad[:8]])
        assert (after[:arr.nbytes] == arr).all() and (after[arr.nbytes:] == 0xAA).all()
    else:
        r, after = scan_device(t, arr, (0, arr.nbytes), clip=probes, adapter_mismatches=per)
        bad = np.nonzero(after[:arr.nbytes] != masked)[0]
        assert bad.size == 0, (bad[:8], after[bad[:8]], masked[bad[:8]])
        assert (after[arr.nbytes:] == 0xAA).all()
        check_clip(r, c)
    t.close()
