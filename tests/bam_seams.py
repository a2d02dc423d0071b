"""
The seam corpus of the BAM record decoder (kernels_bam.hip), in plain Python: the reference of one run
(``run_ref``: what kvq_bam_run_host / kvq_bam_run_device owe for a prefix of a stream), a model of the segment and window
layout of kvq_bam_find / kvq_bam_emit (``layout``), and the streams that put records on the seams -- segment ends, the
4 KiB window of the writer, fake chains inside records, run ends at every byte -- each with the conditions it must meet,
which tests/test_bam_seams_host.py asserts on the CPU before tests/test_gpu_bam_seams.py uses the streams on the GPU.

The reference is written from bam_writer.read and bam_writer.to_fastq (records and their text), not from the order of
kvq_bam_check's tests; ``check`` / ``candidate`` below restate that function only to *predict where the speculation
starts* (the conditions), never to judge a result.
"""
import collections
import functools
import random
import struct

import bam_writer as W
from test_bam_host import RULES, _broken, chain_bait, corpus, mixed_records

WIN = 4096                      # KVQ_BAM_WIN
FIXED = 36                      # KVQ_BAM_FIXED
SWEEP_SIZES = list(range(38, 166)) + [1, 16, 37, 1024, 4096]
KINDS = ['@', 'name', '/', 'mate', 'nl1', 'base', 'nl2', '+', 'nl3', 'qual', 'nl4']

Rec = collections.namedtuple('Rec', 'offset end text written noqual')
Run = collections.namedtuple('Run', 'text end seen written skipped noqual')


# ---- the reference -----------------------------------------------------------------------------------------------

def walk(data):
    """the records of a well-formed stream, each with its text (to_fastq of the header and that record alone)"""
    n_ref, first = W.first_record(data)
    _, recs = W.read(data)
    out = []
    for r, nxt in zip(recs, [q['offset'] for q in recs[1:]] + [len(data)]):
        text = W.to_fastq(data[:first] + data[r['offset']:nxt])
        out.append(Rec(r['offset'], nxt, text, bool(text), bool(text) and r['qual'][:1] == [0xFF]))
    return out


_walks = {}


def walk_cached(data):
    if data not in _walks:
        _walks[data] = walk(data)
    return _walks[data]


def run_ref(data, first, cut):
    """what a run over the prefix data[:cut] of the well-formed stream data owes: the text of the records that end at or
    before cut, and `end`, the smallest record start whose record ends behind cut (cut when no record is cut)"""
    text, end, seen, written, noqual = [], cut, 0, 0, 0
    for r in walk_cached(data):
        if r.offset < first:
            continue
        if r.end > cut:
            end = min(r.offset, cut)
            break
        text.append(r.text); seen += 1; written += r.written; noqual += r.noqual
    return Run(b''.join(text), end, seen, written, seen - written, noqual)


def broken_ref(data, at, bad_end, first, cut):
    """for a stream whose record at `at` (bytes [at, bad_end) as built) breaks a rule: (must_fail, must_succeed, ok) of
    run 1 over data[:cut]; ok: the Run it owes when it succeeds.  Whatever run 1 does, the replay of data[end:] must fail
    naming `at`."""
    ok = run_ref(data[:at], first, min(cut, at))
    return cut >= bad_end, cut <= at, ok


# ---- a restatement of the record rules, for the conditions only ---------------------------------------------------

OK, SHORT, BAD = 0, 1, 2


def check(data, n, limit, n_ref, o):
    """(verdict, next) of the record at o of data[:n], a prefix of a stream that ends at limit"""
    if o + 4 > n:
        return (BAD if n >= limit else SHORT), None
    bs, = struct.unpack_from('<i', data, o)
    if bs < 34 or o + 4 + bs > limit:
        return BAD, None
    if o + FIXED > n:
        return SHORT, None
    ref, pos, lrn, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from('<iiBBHHHiiii', data, o + 4)
    if lrn < 2 or not -1 <= ref < n_ref or not -1 <= nref < n_ref or pos < -1 or npos < -1 or lseq < 0:
        return BAD, None
    if 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
        return BAD, None
    if o + FIXED + lrn > n:
        return SHORT, None
    name = data[o + FIXED:o + FIXED + lrn]
    if name[-1] != 0 or any(c < 33 or c > 126 for c in name[:-1]):
        return BAD, None
    if o + 4 + bs > n:
        return SHORT, None
    return OK, o + 4 + bs


def candidate(data, n, limit, n_ref, o):
    for _ in range(4):
        if o >= n:
            break
        v, nxt = check(data, n, limit, n_ref, o)
        if v != OK:
            return v == SHORT
        o = nxt
    return True


# ---- the layout model --------------------------------------------------------------------------------------------

Seg = collections.namedtuple('Seg', 'k lo hi recs base text')


def layout(data, first, cut, S):
    """the segments of data[first:cut] at segment size S: a record of the chain that lies wholly in the prefix belongs to
    the segment where it starts; a segment's text base is the sum of the texts of the segments in front of it"""
    recs = [r for r in walk_cached(data) if r.offset >= first and r.end <= cut]
    nseg = (cut - first + S - 1) // S
    per = [[] for _ in range(nseg)]
    for r in recs:
        per[(r.offset - first) // S].append(r)
    out, base = [], 0
    for k in range(nseg):
        text = sum(len(r.text) for r in per[k])
        out.append(Seg(k, first + k * S, min(first + (k + 1) * S, cut), per[k], base, text))
        base += text
    return out


def seams(seg, mis):
    """the text offsets (relative to out) where kvq_bam_emit's window of segment seg ends and the next begins"""
    a = ((seg.base + mis) & ~15) - mis
    return [x for x in range(a + WIN, seg.base + seg.text, WIN) if x > seg.base]


def kind(text, j):
    """which of KINDS byte j of one record's text is"""
    nl = [i for i, c in enumerate(text) if c == 10]
    assert len(nl) == 4 and text[0] == 64
    if j == 0:
        return '@'
    if j < nl[0]:
        h = text[:nl[0]]
        if h[-2:] in (b'/1', b'/2') and j >= nl[0] - 2:
            return '/' if j == nl[0] - 2 else 'mate'
        return 'name'
    if j in nl:
        return 'nl%d' % (nl.index(j) + 1)
    if j < nl[1]:
        return 'base'
    if j < nl[2]:
        return '+'
    return 'qual'


def first_passing(data, cut, limit, n_ref, seg):
    """the first offset of the segment that passes the candidate test (None: none does)"""
    for o in range(seg.lo, seg.hi):
        if candidate(data, cut, limit, n_ref, o):
            return o
    return None


def speculation_misled(data, first, cut, S, limit=None):
    """(refuted, emptied): the segments (k > 0) whose first passing offset is no record start of the chain, those the
    chain check must walk again and those it must empty.  Works on malformed streams too: the chain is walked with
    `check` up to its first verdict that is not OK."""
    limit = len(data) if limit is None else limit
    n_ref, _ = W.first_record(data)
    chain, o = set(), first
    while o < cut:
        chain.add(o)
        v, nxt = check(data, cut, limit, n_ref, o)
        if v != OK:
            break
        o = nxt
    refuted, emptied = [], []
    for k in range(1, (cut - first + S - 1) // S):
        seg = Seg(k, first + k * S, min(first + (k + 1) * S, cut), None, 0, 0)
        o = first_passing(data, cut, limit, n_ref, seg)
        if o is not None and o not in chain:
            # a record start of the chain in the segment: the chain check walks it again; none: the host empties it
            (refuted if any(seg.lo <= c < seg.hi for c in chain) else emptied).append(k)
    return refuted, emptied


# ---- the streams -------------------------------------------------------------------------------------------------

TINY = W.record('a', 'A', [30])                # 40 bytes, 9 bytes of text


@functools.lru_cache(None)
def sweep_stream():
    """about 50 short mixed records with runs of the 40-byte record at both ends"""
    mid = [r for r in mixed_records(seed=3, n=60) if len(r) < 700][:36]
    return W.header(3) + b''.join([TINY] * 8 + mid + [TINY] * 8)


@functools.lru_cache(None)
def tiny_stream():
    return W.header(0) + TINY * 40


def sweep_conditions(data, sizes):
    """which of the segment-edge conditions the sizes meet: name -> the sizes that do"""
    n_ref, first = W.first_record(data)
    met = collections.defaultdict(list)
    for S in sizes:
        for seg in layout(data, first, len(data), S):
            if seg.k and any(r.offset == seg.lo for r in seg.recs):
                met['start_at_0'].append(S)
            for d in (1, 2, 3):
                if seg.hi < len(data) and any(r.offset == seg.hi - d for r in seg.recs):
                    met['start_%d_before_end' % d].append(S)
            if seg.hi < len(data) and any(r.offset + 4 <= seg.hi < r.offset + FIXED for r in seg.recs):
                met['fixed_straddles'].append(S)
            if not seg.recs:
                met['passed_over'].append(S)
    return met


def words_from_three_segments(data, S, mis=0):
    """the 16-byte words of out (at misalignment mis) that take bytes from three or more segments"""
    n_ref, first = W.first_record(data)
    owner = {}
    for seg in layout(data, first, len(data), S):
        for x in range(seg.base, seg.base + seg.text):
            owner.setdefault((x + mis) // 16, set()).add(seg.k)
    return [w for w, ks in sorted(owner.items()) if len(ks) >= 3]


PROBES = [dict(name='probe', seq='ACGTTGA', qual=[10, 20, 30, 40, 41, 2, 0], flag=0x10 | 0x40 | 0x1),
          dict(name='probe', seq='GATTACA', qual=None, flag=0x10 | 0x40 | 0x1),
          dict(name='probe', seq='CCGTTGN', qual=[40, 30, 20, 10, 5, 1, 0], flag=0x80 | 0x1)]
WINDOW_D = list(range(1, 100))


@functools.lru_cache(None)
def window_stream(d):
    """fillers, a record whose name is d characters, the three probes, more than 4 KiB behind them: at d == 1 the first
    probe's text ends 2 bytes in front of 4096 - 15, at d == 99 the last probe's begins behind 4096"""
    fill = [W.record('f%d' % i, 'ACGT' * 25, [30 + i % 9] * 100) for i in range(18)]           # 18 x 209 text bytes
    pad = W.record('pad', 'ACGTAC' * 19, [33] * 114)                                            # 237 text bytes
    mover = W.record('m' * d, 'AC', [30, 31])
    tail = [W.record('t%d' % i, 'TTGCA' * 30, [20 + i % 20] * 150, flag=0x40 if i % 2 else 0x80) for i in range(16)]
    data = W.header(0) + b''.join(fill + [pad, mover] + [W.record(**p) for p in PROBES] + tail)
    return data


def window_probe_at(data):
    """[(text offset, text)] of the three probes in the stream"""
    out, t = [], 0
    for r in walk_cached(data):
        if r.text.startswith(b'@probe/'):
            out.append((t, r.text))
        t += len(r.text)
    assert len(out) == 3 and all(len(x[1]) == 27 for x in out)
    return out


def window_cases():
    """the (d, mis) at which a byte of a probe is the last of a window or the first of the next"""
    out = []
    for d in WINDOW_D:
        probes = window_probe_at(window_stream(d))
        for mis in range(16):
            x = WIN - mis
            if any(t <= x - 1 < t + 27 or t <= x < t + 27 for t, _ in probes):
                out.append((d, mis))
    return out


def window_coverage(cases):
    """{(mis, probe, kind, 'last' | 'first')} the cases put on a window seam"""
    got = set()
    for d, mis in cases:
        data = window_stream(d)
        n_ref, first = W.first_record(data)
        seg, = layout(data, first, len(data), len(data) + 1)
        for x in seams(seg, mis):
            for i, (t, text) in enumerate(window_probe_at(data)):
                if t <= x - 1 < t + 27:
                    got.add((mis, i, kind(text, x - 1 - t), 'last'))
                if t <= x < t + 27:
                    got.add((mis, i, kind(text, x - t), 'first'))
    return got


def _fake(n, name='fake'):
    return [W.record('%s%d' % (name, i), 'ACGT' * 5, [30] * 20) for i in range(n)]


def _host(i, payload, **kw):
    return W.record('bait%d' % i, 'ACGTN' * 20, [35] * 100, aux=W.aux_b_bytes(payload), **kw)


def _goods(n, tag='g'):
    return [W.record('%s%d' % (tag, i), 'ACGT' * 10, [30 + i % 5] * 40, flag=(0x40, 0x80, 0x10, 4)[i % 4]) for i in range(n)]


Bait = collections.namedtuple('Bait', 'data at bad_end cut sizes')


@functools.lru_cache(None)
def baits():
    """name -> Bait(stream, offset of its malformed record or None, that record's end, the cut of the run or None,
    segment sizes at which a segment begins inside a bait's array)"""
    hdr = W.header(0)
    out = {}
    g = _goods(12)
    # the fake chain flows back into the true one (the aux array ends where the record does)
    out['flows_back'] = Bait(hdr + b''.join(g[:3] + chain_bait(4) + g[3:]), None, None, None, (300, 1024))
    # a fake chain of 5 records, then one that breaks a rule (l_seq < 0), then bytes that are no record
    bad = bytearray(_fake(1, 'brk')[0]); bad[20:24] = struct.pack('<i', -1)
    breaks = b''.join(_fake(5)) + bytes(bad) + b'\x07' * 90
    out['breaks_a_rule'] = Bait(hdr + b''.join(g[:3] + [_host(i, breaks) for i in range(4)] + g[3:]), None, None, None, (512, 1024))
    # the fifth fake record's block_size reaches over the end of its host into the record behind
    over = bytearray(_fake(1, 'ovr')[0]); over += b'\x00' * 40; over[0:4] = struct.pack('<i', len(over) - 4 + 57)
    shoots = b''.join(_fake(4)) + bytes(over)
    out['overshoots'] = Bait(hdr + b''.join(g[:3] + [_host(i, shoots) for i in range(4)] + g[3:]), None, None, None, (512, 1024))
    # the run ends inside a bait, behind whole fake records
    big = _host(0, b''.join(_fake(30)))
    front = g[:3] + chain_bait(1) + g[3:6]
    data = hdr + b''.join(front + [big] + g[6:])
    at = len(hdr) + sum(len(r) for r in front)
    out['cut_record'] = Bait(data, None, None, at + len(big) - 3 * len(_fake(1)[0]) - 11, (300, 700))
    # a bait directly in front of a truly malformed record
    broken = bytearray(g[7]); broken[8:12] = struct.pack('<i', -2)                          # pos < -1
    front = hdr + b''.join(g[:3] + chain_bait(2))
    out['before_malformed'] = Bait(front + bytes(broken) + b''.join(g[8:]), len(front), len(front) + len(broken), None, (256, 1024))
    return out


@functools.lru_cache(None)
def cut_stream():
    """(stream, [cuts]): a window of a plain record, one with l_seq == 0, a secondary one and one with cigar and aux, cut
    at every byte from the start of the first to the end of the third record behind it; the stream's ends; a 20 kb
    record that spans many segments"""
    rnd = random.Random(12)
    seq = ''.join(rnd.choice('ACGT') for _ in range(20000))
    long_ = W.record('long20k', seq, [rnd.randint(0, 60) for _ in range(20000)], flag=0x10 | 0x80)
    g = _goods(10, 'c')
    win = [W.record('plain', 'ACGTT', [30, 31, 32, 33, 34], flag=0x40),
           W.record('empty', '', []),
           W.record('second', 'ACGTACG', [20] * 7, flag=0x100),
           W.record('cig', 'ACGTNAC', None, flag=0x10, ref=1, pos=77, cigar=[(3, 0), (1, 1), (3, 0)], aux=W.aux_all_types())]
    hdr = W.header(2)
    parts = g[:3] + win + g[3:5] + [long_] + g[5:]
    data = hdr + b''.join(parts)
    first = len(hdr)
    w0 = first + sum(len(r) for r in g[:3])
    w1 = w0 + sum(len(r) for r in win)
    l0 = w1 + sum(len(r) for r in g[3:5])
    cuts = list(range(w0, w1 + 1)) + [first, first + 1] + list(range(len(data) - 3, len(data) + 1))
    cuts += [l0 + 1, l0 + 4, l0 + 35, l0 + 36, l0 + 44, l0 + 5000, l0 + 10043, l0 + 10044, l0 + 20000, l0 + len(long_) - 1, l0 + len(long_)]
    return data, sorted(set(cuts))


Broken = collections.namedtuple('Broken', 'data at bad_end cuts')


@functools.lru_cache(None)
def rule_stream(field, place='plain'):
    """a stream whose record at `at` breaks the rule `field`: test_bam_host._broken, with records in front so that the bad
    record lies in segment 0 ('plain'), in a later segment ('later': 12 records in front), across the end of a segment
    of 256 bytes ('straddle') or directly behind a bait ('bait'); cut at every byte of the bad record and its neighbours"""
    data, at = _broken(field)
    n_ref, first = W.first_record(data)
    good = len(W.record('g0', 'ACGT' * 10, [30] * 40))
    bad_end = len(data) if field == 'past_end' else at + (len(data) - first - 4 * good)
    front = {'plain': [], 'later': _goods(12, 'f'), 'bait': _goods(2, 'f') + chain_bait(1)}.get(place)
    if place == 'straddle':
        # the segment end at first + 256 k falls 20 bytes into the bad record
        front = _goods(3, 'f')
        fill = (256 - 20 - (at - first + sum(len(r) for r in front))) % 256
        front.append(W.record('s', '', [], aux=b'\x00' * ((fill if fill >= 38 else fill + 256) - 38)))       # (aux bytes are not read)
    ins = b''.join(front)
    data = data[:first] + ins + data[first:]
    at += len(ins); bad_end += len(ins)
    lo = at - good
    hi = min(len(data), bad_end + good)
    return Broken(data, at, bad_end, list(range(lo, hi + 1)))


PLACES = {'plain': 4096, 'later': 256, 'straddle': 256, 'bait': 256}           # place -> the segment size it is made for


# ---- the route: a run boundary at a chosen byte -------------------------------------------------------------------

RUN1 = 32 * 65280                                  # the inflated bytes of the first run at KVQ_INFLATE_BATCH_MB=2
PHASES = ['in_block_size', 'at_byte_4', 'in_fixed', 'at_byte_36', 'in_name', 'in_bases', 'in_quals', 'at_last_byte', 'at_end',
          'one_into_next']


def phase_offset(phase, rec_len, lrn, lseq):
    """how far into the probe record the run boundary falls"""
    return {'in_block_size': 2, 'at_byte_4': 4, 'in_fixed': 17, 'at_byte_36': 36, 'in_name': 36 + lrn // 2,
            'in_bases': 36 + lrn + lseq // 4, 'in_quals': 36 + lrn + (lseq + 1) // 2 + lseq // 2, 'at_last_byte': rec_len - 1,
            'at_end': rec_len, 'one_into_next': rec_len + 1}[phase]


MARKER = b'GATTACAGATTACATTGACCATGGCATCAA'                # in the probe and its two neighbours only
ROUTE_READS = 7700
_REC = 275                                         # a 150-base read of synth.reads as a BAM record


@functools.lru_cache(None)
def route_body():
    """(records of the body, index of the probe, the body's virtual text)"""
    from kvarq_amd import synth
    text = synth.reads(synth.genome(), 0, ROUTE_READS, 150).tobytes()
    recs = W.from_fastq(text)
    assert len(recs) == ROUTE_READS and all(len(r) == _REC for r in recs)
    m = (RUN1 - len(W.header(0)) - 38 - _REC - 1) // _REC - 1
    lines = text.split(b'\n')
    for i in (m - 1, m, m + 1):
        bases = lines[4 * i + 1]
        lines[4 * i + 1] = bases[:40 + i - m] + MARKER + bases[40 + i - m + len(MARKER):]
        lines[4 * i + 3] = b'I' * 150
    recs[m - 1:m + 2] = W.from_fastq(b'\n'.join(lines[4 * (m - 1):4 * (m + 2)]) + b'\n')
    body = W.to_fastq(W.header(0) + b''.join(recs))
    assert body.count(MARKER) == 3
    return recs, m, body


def route_stream(phase):
    """(header, records, probe offset, boundary offset inside the probe): a filler record that writes no text moves the
    probe so that the first run's end, RUN1, falls `phase_offset` bytes into it"""
    recs, m, _ = route_body()
    hdr = W.header(0)
    off = phase_offset(phase, _REC, 14, 150)
    k = RUN1 - off - len(hdr) - 38 - _REC * m
    assert 0 <= k < 3 * _REC
    filler = W.record('f', '', [], aux=b'\x00' * k)                 # (aux bytes are not read)
    probe = len(hdr) + len(filler) + _REC * m
    assert probe + off == RUN1
    return hdr, [filler] + recs, probe, off
