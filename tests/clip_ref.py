"""
The adapter clip of a scan (include/kvarq_hip.h) in plain Python on top of ``adapt_ref.per_record`` --
``mask`` and the eight words --, the texts that take the kernel's stores and the trim behind them to their seams, and for every
text a CENSUS, asserted before any comparison, that it reaches the seams it is built for.  Not a test module.

 * ``stores``: the first byte of the score line on every address residue modulo 16, CLIP = 0 .. 47 and S - CLIP = 1 .. 48 (every
   first address modulo 16 with every length: what the byte, dword and 16-byte stores of a quarter-wave depend on), the seams of
   the search's rounds, score lines shorter and longer than their bases line, '\\r' on either line, tails, two probes, 12 kb lines;
 * ``reveal``: records of ``trim_matrix``'s template whose bases turn into adapter at an insert length: every record whose MASKED
   trim leaves ``minreadlength`` is a hit that carries (file_pos, readlength) -- another mask, another set;
 * ``redo``: the same with long records that their tiles leave to the redo; ``quirk``: a text whose speculated record split fails;
 * ``none``: no probe anywhere.
"""
import functools
import random

import numpy as np

import adapt_ref as A
import cases
import kernel_matrix as KM
import profile_ref as R
import trim_matrix as TM
from kvarq_amd import synth

C_N, C_RECORDS, C_CLIPPED, C_MASKED, C_BASES_CUT, LEN = 0, 1, 2, 3, 4, 8
# the probes of a run with N of them: P12 first, which the texts plant
PROBES = {1: [A.P12], 2: [A.P12, A.P32], 4: [A.P12, A.P32, A.P8, A.PERIODIC],
          8: [A.P12, A.P32] + [p for p in A.EIGHT if p not in (A.P12, A.P32)]}
CFG = dict(KM.CONFIGS[8])                                   # Amin '.', minreadlength 25
AMIN = ord('.')
QUIRK_CFG = dict(cases.PRODUCT)


def per_record(text, chunk_off, probes):
    """for every record (n2, L, CLIP, S)"""
    text = bytes(text)
    co = [int(c) for c in chunk_off]
    out = []
    for (n0, _, n2, n3), (start, L, _, _, clip, _) in zip(R.records_of(text, co), A.per_record(text, co, probes)):
        assert start == n0 + 1
        S = n3 - n2 - 1
        if S and text[n3 - 1] == 13:
            S -= 1                                            # a trailing '\r' is not part of its line
        out.append((n2, L, clip, S))
    return out


def mask(text, chunk_off, probes, into=None):
    """(MASK(text), the eight words); ``into``: add to them, as kvq_clip_host does"""
    out = bytearray(text)
    w = np.zeros(LEN, dtype=np.int64) if into is None else into
    w[C_N] = len(probes)
    for n2, L, clip, S in per_record(text, chunk_off, probes):
        w[C_RECORDS] += 1
        if clip < L:
            w[C_CLIPPED] += 1; w[C_MASKED] += max(0, S - clip); w[C_BASES_CUT] += L - clip
            if S > clip:
                out[n2 + 1 + clip:n2 + 1 + S] = b'!' * (S - clip)
    return bytes(out), w


def record_ends(text):
    return [n3 + 1 for _, _, _, n3 in R.records_of(bytes(text), [0, len(text)])]


# ---- stores ------------------------------------------------------------------------------------------------------------------

class _Stores(object):
    def __init__(self):
        self.parts, self.at, self.rng, self.kinds = [], 0, np.random.RandomState(190), []

    def add(self, bases, scores, kind, residue=None, nl_b=b'\n', nl_s=b'\n'):
        """a record whose score line begins at an offset that is ``residue`` modulo 16 (the name line's length sets it)"""
        residue = len(self.parts) % 16 if residue is None else residue
        fixed = self.at + 2 + len(bases) + len(nl_b) + 2       # '@' '\n' bases nl '+' '\n' in front of the scores, but for the name
        nlen = (residue - fixed) % 16 or 16
        r = b'@' + b'n' * nlen + b'\n' + bases + nl_b + b'+\n' + scores + nl_s
        assert (self.at + len(r) - len(nl_s) - len(scores)) % 16 == residue
        self.parts.append(r); self.at += len(r); self.kinds.append(kind)

    def scores(self, n):
        return self.rng.choice(np.frombuffer(b'IIII5#~', dtype=np.uint8), n).tobytes() if n else b''

    def planted(self, clip, L, probe=A.P12):
        return A.filler(self.rng, clip) + probe + A.filler(self.rng, L - clip - len(probe))


@functools.lru_cache(maxsize=None)
def stores_text():
    b = _Stores()
    for clip in range(48):
        for rem in range(1, 49):
            i = len(b.parts)
            b.add(b.planted(clip, clip + 12 + i % 5), b.scores(clip + rem), 'sweep')
    for clip in (223, 224, 225, 447, 448, 449):
        b.add(b.planted(clip, clip + 32), b.scores(clip + 32), 'seam')
        b.add(b.planted(clip, clip + 40, A.P32), b.scores(clip + 40), 'seam')
    for S in (30, 29, 10, 1, 0):                                                    # S <= CLIP: nothing to mask, still clipped
        b.add(b.planted(30, 60), b.scores(S), 'short')
    for nl_b, nl_s in ((b'\r\n', b'\n'), (b'\n', b'\r\n'), (b'\r\n', b'\r\n')):
        for clip, L in ((20, 50), (0, 12), (38, 50)):
            b.add(b.planted(clip, L), b.scores(L), 'cr', nl_b=nl_b, nl_s=nl_s)
        b.add(A.filler(b.rng, 30) + A.P12[:8], b.scores(38), 'cr', nl_b=nl_b, nl_s=nl_s)          # a tail in front of a '\r'
        b.add(b.planted(10, 40), b'', 'cr', nl_b=nl_b, nl_s=nl_s)                                # S == 0 once the '\r' is gone
    for t in (6, 7, 11):
        for L in (t, 40, 150, 300):
            b.add(A.filler(b.rng, L - t) + A.P12[:t], b.scores(L), 'tail')
    b.add(A.filler(b.rng, 45) + A.P12[:5], b.scores(50), 'tail')                    # t = 5: none
    for gap in (0, 23, 200):                                                        # the later probe's FIRST is the smaller
        b.add(A.filler(b.rng, 5) + A.P32 + A.filler(b.rng, gap) + A.P12 + A.filler(b.rng, 10), b.scores(59 + gap), 'two')
    for c in (3, 4095, 4096, 4097, 12000 - 12):
        b.add(b.planted(c, 12000), b.scores(12000), 'long')
    b.add(A.filler(b.rng, 12000), b.scores(12000), 'long')
    for L in (0, 1, 50, 150):                                                       # unclipped among them
        b.add(A.filler(b.rng, L), b.scores(L), 'plain')
    b.add(b.planted(100, 112), b.scores(112), 'last')                               # flush with its line's end, the text's last record
    return b''.join(b.parts), tuple(b.kinds)


def stores_census():
    text, kinds = stores_text()
    recs = per_record(text, [0, len(text)], PROBES[2])
    assert len(recs) == len(kinds) and 2000 <= len(recs) <= 5000
    c = dict(stores=set(), residues=set(), clips=set(), rems=set(), s_lt=0, s_gt=0, s_le_clip=0, s_zero=0, unclipped=0)
    for (n2, L, clip, S), kind in zip(recs, kinds):
        c['residues'].add((n2 + 1) % 16)
        if clip >= L:
            c['unclipped'] += 1
            continue
        c['clips'].add(clip)
        c['s_lt'] += S < L; c['s_gt'] += S > L; c['s_le_clip'] += S <= clip; c['s_zero'] += S == 0
        if S > clip:
            c['stores'].add(((n2 + 1 + clip) % 16, S - clip)); c['rems'].add(S - clip)
    assert c['residues'] == set(range(16))
    assert c['stores'] >= {(a, n) for a in range(16) for n in range(1, 49)}         # every first address with every length
    assert c['clips'] >= set(range(48)) | {223, 224, 225, 447, 448, 449, 3, 4095, 4096, 4097, 11988}
    assert c['rems'] >= set(range(1, 49)) | {11997, 12}
    assert c['s_lt'] > 100 and c['s_gt'] > 100 and c['s_le_clip'] >= 5 and c['s_zero'] >= 3 and c['unclipped'] >= 5
    by_kind = lambda k: [r for r, kind in zip(recs, kinds) if kind == k]
    assert sorted(L - clip for _, L, clip, _ in by_kind('tail')) == [0] + [6] * 4 + [7] * 4 + [11] * 4
    assert [clip for _, _, clip, _ in by_kind('two')] == [5, 5, 5]
    text_b = bytes(text)
    crs = [(text_b[n2 - 3:n2 - 2] == b'\r', text_b[n2 + S + 1:n2 + S + 2] == b'\r') for n2, _, _, S in by_kind('cr')]
    assert {(True, False), (False, True), (True, True)} <= set(crs)
    assert text_b.endswith(A.P12 + b'\n+\n' + text_b[-113:-1] + b'\n')
    return c


# ---- reveal --------------------------------------------------------------------------------------------------------------------

REVEAL_L = 150
REVEAL_INS = (0, 1, 24, 25, 26, 31, 40, 57, 60, 75, 90, 100, 110, 123, 124, 130, 138)
FORMS = ('good', 'dip', 'straddle', 'equal', 'longer')


def reveal_scores(form, c, L=REVEAL_L):
    """the score line of a record whose adapter begins at c: 'I' is a good score at Amin '.', '#' a bad one"""
    pat = [1] * L
    if form == 'dip' and c >= 30:                         # a dip in front of the adapter: unmasked, the best run lies behind it
        pat[c // 2 + 3] = 0
    elif form == 'straddle' and c >= 31:                  # the best run straddles CLIP
        pat[c - 30] = 0; pat[min(c + 20, L - 1)] = 0
    elif form in ('equal', 'longer') and 26 <= c <= L - 28:
        r = 26                                            # a run of r in front of CLIP and one of r (r + 1: 'longer') behind it
        pat = [0] * L
        pat[c - r:c] = [1] * r
        pat[c + 1:c + 1 + r + (form == 'longer')] = [1] * (r + (form == 'longer'))
    return bytes(ord('I') if v else ord('#') for v in pat)


class _Reveal(object):
    """records with trim_matrix's header: a record of 150 bases has synth.record_bytes(150) bytes, as trim_matrix.redo_text's"""

    def __init__(self, seed):
        self.T, self.P = TM.template(), TM.probe()
        self.rng, self.nrng = random.Random(seed), np.random.RandomState(seed)
        self.parts, self.nbytes, self.ins, self.read_off = [], 0, [], []

    def add(self, bases, scores, c):
        head = (TM.HEADER_FMT % len(self.parts)).encode()
        self.read_off.append(self.nbytes + len(head)); self.ins.append(c)
        self.parts.append(head + bases + b'\n+\n' + scores + b'\n'); self.nbytes += len(self.parts[-1])

    def short(self):
        n = len(self.parts)
        c = REVEAL_INS[n % len(REVEAL_INS)]
        form = FORMS[(n // len(REVEAL_INS)) % len(FORMS)]
        a = self.rng.randrange(0, TM.TEMPLATE_LEN - c + 1)
        self.add(self.T[a:a + c] + A.P12 + A.filler(self.nrng, REVEAL_L - c - 12), reveal_scores(form, c), c)

    def long(self, Q, c):
        """random bases, trim_matrix's probe inside the part in front of the adapter at c, good scores throughout"""
        bases = bytearray(self.rng.choice(b'ACGT') for _ in range(Q))
        bases[c // 2:c // 2 + TM.PROBE_LEN] = self.P
        bases[c:c + 12] = A.P12
        self.add(bytes(bases), b'I' * Q, c)

    def text(self):
        return b''.join(self.parts)


@functools.lru_cache(maxsize=None)
def reveal_text():
    b = _Reveal(191)
    while b.nbytes < (128 << 10) + 8192 + 3 * TM.TILE_OWNS:
        b.short()
    return b.text(), tuple(b.read_off), tuple(b.ins)


REDO_LONG = [(5000, 2000), (9000, 8000), (12000, 4096), (6000, 5988)]


@functools.lru_cache(maxsize=None)
def redo_text():
    """as trim_matrix.redo_text: a head of short records, then long records that start inside their chunk's first tile and end
    beyond its look-ahead -> (text, read offsets, insert lengths, chunk offsets)"""
    b = _Reveal(192)
    rb = synth.record_bytes(REVEAL_L)
    co = [0]
    while b.nbytes < (128 << 10) + 8192:
        b.short()
    for Q, c in REDO_LONG:
        co.append(b.nbytes)
        before = 108 if 108 * rb + 2 * Q + 25 > TM.TILE_OWNS + TM.LOOKAHEAD + 160 else 120
        assert before * rb < TM.TILE_OWNS - 160 and before * rb + 2 * Q + 25 > TM.TILE_OWNS + TM.LOOKAHEAD + 160
        for _ in range(before):
            b.short()
        b.long(Q, c)
        for _ in range(10):
            b.short()
    co.append(b.nbytes)
    return b.text(), tuple(b.read_off), tuple(b.ins), tuple(co)


def revealed(text, read_off, chunk_off, probes, masked=True):
    """{(file_pos, readlength)} of the records whose trim -- of the masked score line, or of the line as it lies -- leaves
    minreadlength or more, and the trims themselves"""
    src = mask(text, chunk_off, probes)[0] if masked else bytes(text)
    trims = [TM.trim(src[n2 + 1:n3], AMIN) for _, _, n2, n3 in R.records_of(src, [int(c) for c in chunk_off])]
    assert len(trims) == len(read_off)
    return set((off + s, ln) for off, (s, ln) in zip(read_off, trims) if ln >= CFG['minreadlength']), trims


def reveal_census(which='reveal'):
    if which == 'reveal':
        text, read_off, ins = reveal_text(); co = [0, len(text)]
    else:
        text, read_off, ins, co = redo_text()
    assert read_off[1] - read_off[0] == synth.record_bytes(REVEAL_L)      # (what redo_text's placement of the long records counts on)
    recs = per_record(text, co, PROBES[2])
    assert [clip for _, _, clip, _ in recs] == list(ins)                  # the adapter begins where the builder put it, nowhere earlier
    want, masked = revealed(text, read_off, co, PROBES[2])
    _, plain = revealed(text, read_off, co, PROBES[2], masked=False)
    differ = sum(a != b for a, b in zip(masked, plain))
    assert 4 * len(want) >= len(recs) and differ >= 50, (len(want), len(recs), differ)
    assert sum(ln == 0 for _, ln in masked) >= 5 and sum(ln == 1 for _, ln in masked) >= 5      # (the histogram's low bins: a mask one short at its end shows there)
    return dict(records=len(recs), reveal=len(want), differ=differ)


# ---- a text whose speculated record split fails (tests/test_gpu_parity.py: _quirk_text with every=True), with adapters ---------

@functools.lru_cache(maxsize=None)
def quirk_text():
    rng = random.Random(193)
    nrng = np.random.RandomState(193)
    recs = []
    for i in range(4000):
        bases = cases.randseq(rng, rng.randint(60, 200))
        if i % 2 == 0:
            at = rng.randint(1, len(bases) - 1)
            bases = (bases[:at] + cases.QUIRK_SEQ)[:230]
        if i % 3 == 0:
            c = rng.randint(30, len(bases))
            bases = bases[:c] + A.P12.decode() + A.filler(nrng, rng.randint(0, 40)).decode()
        bases = ('@' if i % 7 == 0 else '+') + bases[1:]
        q = '@' + ''.join(rng.choice('@+IIII') for _ in bases[1:])
        recs.append(cases.rec('r%d' % i, bases, q))
    return b''.join(recs)


def quirk_seqs():
    return synth.both_strands([cases.QUIRK_SEQ.encode()])


@functools.lru_cache(maxsize=None)
def none_text():
    return A.none_text()[0]
