"""
The per-cycle counts of a FastQ text (include/kvarq_hip.h) as a plain Python statement of their
definition: the yardstick of tests/test_cycles_host.py (the CPU twin) and tests/test_gpu_cycles.py (the kernel).

They cover the records the profile covers (``profile_ref.records_of``).  Cycle p of a record is byte p of its bases line
and, independently, byte p of its score line; cycles 0 .. 1023 are counted, bytes beyond nowhere.  One flat int64 array:
score[p][b] at p * 256 + b, base[p][b] at 1024 * 256 + p * 256 + b.
"""
import numpy as np

import profile_ref as R

CYCLES = 1024
LEN = 2 * CYCLES * 256


def cycles(text, chunk_off=None, into=None):
    """the flat int64 array; ``into``: add to it, as kvq_cycles_host does"""
    text = bytes(text)
    if chunk_off is None:
        from oracle import oracle as O
        chunk_off = O.chunk_offsets(text) if text else [0]
    out = np.zeros(LEN, dtype=np.int64) if into is None else into
    arr = np.frombuffer(text, dtype=np.uint8)
    for n0, n1, n2, n3 in R.records_of(text, [int(c) for c in chunk_off]):
        for at, a, b in ((0, n2 + 1, n3), (CYCLES * 256, n0 + 1, n1)):
            line = arr[a:min(b, a + CYCLES)]
            np.add.at(out, at + np.arange(len(line)) * 256 + line, 1)
    return out


def score_facts(text, chunk_off):
    """(the longest score line, the records with a non-empty score line): what the profile does not hold"""
    lens = [n3 - n2 - 1 for _, _, n2, n3 in R.records_of(bytes(text), [int(c) for c in chunk_off])]
    return max(lens, default=0), sum(1 for q in lens if q > 0)


def check_identities(cycles, profile_words, facts=None):
    """the three identities of the header, each across two kernels (the cycles against the profile of the same records);
    ``facts``: ``score_facts`` of the text, where the caller has it"""
    score, base = cycles[:CYCLES * 256].reshape(CYCLES, 256), cycles[CYCLES * 256:].reshape(CYCLES, 256)
    w = profile_words
    assert cycles.shape == (LEN,) and (cycles >= 0).all()
    # 1: the bases lines that reach cycle p are the lines longer than p
    raw = w[R.RAW_LENGTHS:R.RAW_LENGTHS + R.RAW_BINS]
    assert (base.sum(axis=1) == raw[::-1].cumsum()[::-1][1:]).all()
    # 2: no byte more than the profile counts, and every byte where no line of the kind has more than 1024
    score_bytes, base_bytes = w[R.SCORE_BYTES:R.SCORE_BYTES + 256], w[R.BASE_BYTES:R.BASE_BYTES + 256]
    assert (score.sum(axis=0) <= score_bytes).all() and (base.sum(axis=0) <= base_bytes).all()
    if w[R.LONGEST] - 1 <= CYCLES:
        assert (base.sum(axis=0) == base_bytes).all()
    if facts is not None and facts[0] <= CYCLES:
        assert (score.sum(axis=0) == score_bytes).all()
    # 3: cycle 0 of the scores is reached by the records with a non-empty score line
    assert score[0].sum() <= w[R.RECORDS]
    if facts is not None:
        assert score[0].sum() == facts[1]
    # (every line reaches the cycles in front of the last one it reaches)
    assert (np.diff(score.sum(axis=1)) <= 0).all() and (np.diff(base.sum(axis=1)) <= 0).all()
