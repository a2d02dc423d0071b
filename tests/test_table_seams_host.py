"""
The tables and texts of tests/table_seams.py are what they claim to be (no GPU): every record's trimmed read gives on every
one of its targets what the plain statement match_matrix.alignments planned, the oracle finds the same for every record
(none is left out), every class -- family x cell x dead leading blocks x side x byte kind -- has a record that hits and a
twin that does not, and the families reach what they were built for: the light reads stay within 64 candidates, the heavy
ones have more hits and more work items than a wave's queues hold, reads have valid diagonals with different canonical
discoverers, and the F tables put a seeded sequence across offset 2^20 and sequence numbers on both sides of 2^16.
"""
import pytest

import kernel_matrix as KM
import match_matrix as MM
import table_seams as TS
import trim_matrix as TM
from kvarq_amd import synth
from oracle import oracle as O

MAKES, make_of = TS.MAKES, TS.make_of


def ident(v):
    return str(v)


def test_the_restatement_of_the_canonical_order_on_its_own_definition():
    """Index on a table of one sequence, small enough to check by eye (K = 5, maxerrors 1, stride 2: pitch 6)"""
    q = b'ACGTTGCATCAGGAT'
    ix = TS.Index([q], 5, 1)
    assert (ix.stride, ix.pitch) == (2, 6) and sum(ix.anc.values()) == 4 and sum(ix.all.values()) == 11 and ix.entries == 15
    # (a tail block that is a head block too is looked up once)
    assert ix.fixed(16) == [0, 5, 11, 6] and ix.fixed(15) == [0, 5, 10] and ix.fixed(10) == [0, 5] and ix.fixed(12) == [0, 5, 7, 2]
    c = TS.codes
    assert c(b'ACGTNacgt.') == bytes([0, 1, 3, 2, 3, 0, 1, 3, 2, 3])
    # the sequence as the read: head block 0; with that block broken: head block 1; with both: the tail block at 10
    assert ix.discoverer(c(q), c(q), 0) == ('F', 0)
    assert ix.discoverer(c(b'T' + q[1:]), c(q), 0) == ('F', 5)
    assert ix.discoverer(c(b'T' + q[1:5] + b'A' + q[6:]), c(q), 0) == ('F', 10)
    # the sequence inside a read of 40: no fixed block of the read lies on it, anchor block 0 of the copy with the
    # diagonal's residue discovers it, block 1 when a mismatch kills that
    read = b'T' * 13 + q + b'T' * 12
    assert ix.discoverer(c(read), c(q), -13) == ('A', 1)
    assert ix.discoverer(c(read[:14] + b'A' + read[15:]), c(q), -13) == ('A', 7)
    assert ix.discoverer(c(b'T' * 40), c(q), -13) is None
    assert ix.candidates(read) == 11 and ix.work_items(q) == 2 + 3


@pytest.mark.parametrize('m', MAKES, ids=TS.make_id)
def test_the_statement_and_the_oracle_find_on_every_record_what_was_planned(m):
    w = make_of(*m)
    amin = ord(w.cfg['Amin'])
    raw = w.data.tobytes()
    for i, sp in enumerate(w.specs):
        assert sp.n == i and TM.trim(sp.scores, amin) == (sp.lead, len(sp.read)), sp
        at = w.starts[i]
        assert raw[at:raw.index(b'\n', at)].split(b' ')[0] == b'@T%s.%d' % (w.fam.encode(), i)
        read = raw[w.reads[i]:w.reads[i] + len(sp.read)]
        assert read == sp.read and w.spec_at(w.reads[i]) == i and w.ends[i] - at >= TS.PAD_TO
        assert sp.target in sp.targets
        for t in sp.targets:
            assert TS.planned(read, w.seqs[t], w.cfg) == sp.plan[t], (sp, t)
        aimed = [(p, ln) for p, ln in sp.plan[sp.target] if p == sp.d]
        assert bool(aimed) == sp.hit == (sp.nmis <= w.e and len(read) >= w.mrl), sp
        if aimed:                                                  # the aimed alignment holds exactly these mismatches
            p, ln = aimed[0]
            hb, q = MM.hit_bytes(read, p, ln), w.seqs[sp.target][max(0, p):max(0, p) + ln]
            a = -p if p < 0 else 0
            assert [a + j for j in range(ln) if hb[j] != q[j]] == list(sp.offs), sp
    assert w.spec_at(w.cut) == len(w.specs) // 2 and 0 < w.cut < w.data.nbytes
    # the oracle: every record, none left out
    o = O.scan_memory(w.data, w.seqs, fold=True, nthreads=16, **w.cfg)
    got, want = w.by_spec(o['hits']), w.planned()
    for i, sp in enumerate(w.specs):
        for t in sp.targets:
            assert got.get((i, t), []) == want.get((i, t), []), (sp, t, got.get((i, t)))
    assert set(got) == set(want) and o['stats']['records_parsed'] == len(w.specs)


@pytest.mark.parametrize('m', MAKES, ids=TS.make_id)
def test_every_class_has_a_record_that_hits_and_a_twin_that_does_not(m):
    w = make_of(*m)
    full = [sp for sp in w.specs if not sp.trimmed]
    for cls in w.classes():
        of = [sp for sp in full if sp.cls == cls and sp.nmis >= w.e]
        assert any(sp.hit and sp.nmis == w.e for sp in of) and any(not sp.hit and sp.nmis == w.e + 1 for sp in of), cls
    # a twin has the mismatches of its record and one more
    for a, b in zip(w.specs, w.specs[1:]):
        if a.nmis == w.e and b.nmis == w.e + 1 and b.n == a.n + 1:
            assert set(a.offs) < set(b.offs) and (a.target, a.d, a.side, a.dead) == (b.target, b.d, b.side, b.dead)
    # the dead blocks: one mismatch each, on the first base of a block and on the last; the block behind them untouched
    edges = set()
    for sp in full:
        d, k = sp.d, w.k
        rl = len(sp.read)
        blocks = ([j * k for j in range(w.e + 1)] if sp.side == 'head' else [rl - (j + 1) * k for j in range(w.e + 1)] if sp.side == 'tail'
                  else [j * w.pitch + d % w.stride - d for j in range(w.e + 1)])
        for j in range(sp.dead):
            inside = [o - blocks[j] for o in sp.offs if blocks[j] <= o < blocks[j] + k]
            assert len(inside) == 1 and inside[0] in (0, k - 1), sp
            edges.add(inside[0])
        assert not any(blocks[sp.dead] <= o < blocks[sp.dead] + k for o in sp.offs), sp
    assert edges == {0, w.k - 1}
    assert set(sp.kind for sp in full) == set(TS.KINDS)
    wrote = set(sp.read[o] for sp in w.specs for o in sp.offs)
    assert wrote & set(b'ACGT') and wrote & set(b'acgtN.') and wrote & set(range(128, 256)), sorted(wrote)


@pytest.mark.parametrize('c,s', TS.R_CELLS, ids=ident)
def test_the_repeat_tables_and_what_their_texts_reach(c, s):
    light, heavy = TS.repeats(c, s, False), TS.repeats(c, s, True)
    assert light.seqs == heavy.seqs and light.cfg == TS.CONFIGS[c]
    k, e = light.k, light.e
    seqs = light.seqs
    n = len(seqs) // 2
    # every unit cut to the spans of the strides the cell allows, to 64 and to 100; both strands; a repeat first and last
    lens = sorted(set([KM.span_of(k, e, st) for st in TS.STRIDES if st >= s] + [64, 100]))
    assert seqs[:n] == [(u * 100)[:L] for u in TS.UNITS for L in lens] and seqs[n:] == [synth.revcomp(q) for q in seqs[:n]]
    assert sorted(len(u) for u in TS.UNITS) == [1, 2, 3, 4, 5, 7, 8, 16] and k in (5, 6, 8) and {k, KM.pitch_of(k, s)} <= {1, 2, 3, 4, 5, 6, 7, 8, 16}
    assert KM.index_stride(seqs, k, e) == s == light.stride and min(len(q) for q in seqs) == KM.span_of(k, e, s)
    assert seqs[0] == b'A' * lens[0] and seqs[-1] == synth.revcomp((TS.UNITS[-1] * 100)[:100])
    assert seqs[n + 3 * len(lens) + lens.index(64)] == seqs[3 * len(lens) + lens.index(64)] == b'ACGT' * 16      # (a twin of its own)
    # the product's cell lands on the halving kernel, the others on the draining ones (K < 8)
    assert (k == 8 and not KM.index_dense(seqs, k, e, s)) or k < 8
    # light: within the bound, 25 to 60 bases of a repeat at every phase of every unit
    ix = light.index
    assert max(ix.candidates(sp.read) for sp in light.specs) <= TS.LIGHT_BOUND < TS.ST_QW
    phases = set((sp.unit, sp.phase) for sp in light.specs if not sp.trimmed)
    assert phases == set((u, ph) for u in TS.UNITS for ph in range(len(u))), sorted(phases)
    assert all(len(sp.read) <= 60 + 40 for sp in light.specs)
    # heavy: pure repeat reads of 150 bases and one pair of 1500; more hits than 64 and more work items than a queue holds
    assert sorted(set(len(sp.read) for sp in heavy.specs if not sp.trimmed)) == [150, 1500]
    for sp in heavy.specs:
        clean = bytearray(sp.read)
        for o in sp.offs:
            clean[o] = 0
        u = sp.unit
        assert any(all(b in (0, x) for b, x in zip(clean, (u * (len(clean) // len(u) + 2))[ph:])) for ph in range(len(u))), sp
    hits = [sum(len(pl) for pl in sp.plan.values()) for sp in heavy.specs]
    assert max(hits) > 64 and max(heavy.index.work_items(sp.read) for sp in heavy.specs) > TS.ST_Q2W
    # both: a read with valid diagonals on one sequence that different seeds discover
    for w in (light, heavy):
        assert sum(w.differing(sp) for sp in w.specs) >= 10
    # the reads whose head and tail blocks coincide
    for w in (light, heavy):
        got = sorted(set(len(sp.read) for sp in w.specs if sp.trimmed))
        assert got == list(TS.TRIMMED.get(k, ())), got
        assert all(len(sp.read) % k == 0 for sp in w.specs if sp.trimmed)
        assert k == 6 or any(sp.hit for sp in w.specs if sp.trimmed)


@pytest.mark.parametrize('c,s', TS.T_CELLS, ids=ident)
def test_the_tables_of_twins_and_nested_sequences(c, s):
    w = TS.twins(c, s)
    k, e, names, seqs = w.k, w.e, w.names, w.seqs
    n = len(names)
    nr = names.index
    assert w.stride == s and all(w.seeded) and len(seqs) == 2 * n
    assert seqs[nr('twin')] == seqs[nr('twin-far')] and nr('twin-far') - nr('twin') == n - 1
    base = seqs[nr('twin')]
    assert base.startswith(seqs[nr('prefix')]) and base.endswith(seqs[nr('suffix')]) and seqs[nr('infix')] in base[1:-1]
    span = KM.span_of(k, e, s)
    for name, lo, hi in (('block0', 0, k), ('blocke', e * w.pitch, e * w.pitch + k), ('outside', span, 80)):
        a, b = seqs[nr(name)], seqs[nr(name + "'")]
        diff = [i for i in range(80) if a[i] != b[i]]
        assert len(diff) == 1 and lo <= diff[0] < hi, (name, diff)
    assert seqs[nr('palindrome')] == synth.revcomp(seqs[nr('palindrome')]) == seqs[n + nr('palindrome')]
    assert seqs[nr('g-rich')].count(b'G') >= 48 and seqs[nr('a64')] == b'A' * 64
    # the G-rich sequence holds the last code there is: its entries close ent[]
    assert TS.codes(b'G' * k) == bytes([3] * k) and b'G' * k in seqs[nr('g-rich')]
    # every named sequence is aimed at with a hit; twins, nested sequences and the palindrome hit beside it
    aimed = set(sp.target for sp in w.specs if sp.hit)
    assert aimed >= set(nr(x) for x in names if x != 'setter') | {n + nr('twin-far'), n + nr('g-rich')}
    also = set((sp.target, t) for sp in w.specs for t, pl in sp.plan.items() if pl and t != sp.target)
    assert (nr('twin'), nr('twin-far')) in also and (nr('twin-far'), nr('twin')) in also
    assert (nr('palindrome'), n + nr('palindrome')) in also and (nr('infix'), nr('twin')) in also and (nr('block0'), nr("block0'")) in also
    # ... and one of a pair hits where the other does not: the pair's difference is the mismatch that decides
    assert any(bool(sp.plan[nr(x)]) != bool(sp.plan[nr(x + "'")]) for sp in w.specs for x in ('block0', 'blocke', 'outside'))
    assert sum(w.differing(sp) for sp in w.specs) >= 1


def test_the_table_that_fills_the_offset_field():
    w = TS.f_offset()
    off = TS.offsets_of(w.seqs)
    assert [len(q) for q in w.seqs] == [4095] * 256 + [255, 60, 60, 60, 60] and w.cfg == KM.CONFIGS[8]
    assert off[256] == (1 << 20) - 256 and off[257] == (1 << 20) - 1 < (1 << 20) < off[258] == (1 << 20) + 59
    assert w.seeded == [True] * 258 + [False] * 3 and all(KM.seedable(q, 8, 2) for q in w.seqs)      # (refused for the offset alone)
    # the index of all positions alone has more entries than 2^20, and the last of them belong to G x 8 of the straddling sequence
    entries = sum(len(q) - 8 + 1 for q in w.seqs[:258]) + 258 * 3 * w.stride
    assert (1 << 20) < entries < (1 << 22) and w.stride == 8
    assert w.seqs[257].endswith(b'G' * 30)
    assert sum(1 for sp in w.specs if sp.target == 257 and sp.hit and sp.read.startswith(b'G' * 8)) >= 2
    aimed = lambda hit: set(sp.target for sp in w.specs if sp.hit == hit)
    assert aimed(True) == aimed(False) == {0, 128, 255, 256, 257, 258, 259}
    assert 100 <= len(w.specs) <= 130


def test_the_table_that_fills_the_number_field():
    w = TS.f_number()
    off = TS.offsets_of(w.seqs)
    assert len(w.seqs) == 87500 and set(len(q) for q in w.seqs) == {12} == {KM.span_of(5, 1, 2)} and w.cfg == KM.CONFIGS[5]
    assert off[87381] == 1048572 < (1 << 20) <= off[87382] == 1048584
    assert w.seeded == [True] * 87382 + [False] * 118 and (w.k, w.stride) == (5, 2)
    assert 87382 * (2 * 2 + 8) < (1 << 22)
    for t in TS.FNumber.PLANTED:
        of = [sp for sp in w.specs if sp.target == t]
        assert set(sp.nmis for sp in of if sp.hit) == {0, 1} and any(sp.nmis == 2 and not sp.hit for sp in of), t
    assert all(len(sp.read) == 100 for sp in w.specs) and 30 <= len(w.specs) <= 48


def test_the_census_names_every_text():
    ws = [make_of(*m) for m in MAKES]
    lines = TS.census_lines(ws)
    assert len(lines) == len(MAKES) == 23 and all('records' in ln for ln in lines)
    # the share of records left out is zero: every spec made is in its text
    assert all(len(w.starts) == len(w.specs) for w in ws)
