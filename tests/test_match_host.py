"""
The texts of tests/match_matrix.py are what they claim to be (no GPU): the plain statement of workhorse.c:1112-1174
finds on every spec's read and target exactly the hits the spec planned, the oracle finds the same in every text, for
every spec, and every cell holds every geometry, seam class and byte kind.
"""
import itertools

import pytest

import match_matrix as MM
import trim_matrix as TM
from oracle import oracle as O

_oracle = {}


def oracle_of(name, bg):
    w = MM.cell(name)
    if (name, bg) not in _oracle:
        _oracle[name, bg] = O.scan_memory(w.texts[bg].data, w.seqs, fold=True, nthreads=16, **w.cfg)
    return _oracle[name, bg]


TEXTS = [(name, bg) for name in MM.CELLS for bg in MM.BACKGROUNDS[name]]
GEOMETRIES = (['A', 'B', 'Cs', 'A-mo', 'A-mo-1', 'A-max', 'B-mo', 'B-mo-1', 'B-max', 'BC', 'Cr-0', 'Cr-end', 'Ceq', 'Cs-0', 'Cs-mid',
               'G-rl=mo', 'G-rl=mo+1', 'G-seql=mo', 'big-A', 'big-B', 'big-C', 'keep-in-read', 'keep-eq'] + ['Cr-r%d' % r for r in range(8)])


def test_the_statement_on_the_four_loops():
    """alignments() on pairs small enough to check by eye"""
    cfg = dict(maxerrors=1, minoverlap=3)
    q = b'ACGTTGCA'
    assert MM.alignments(b'TTTTACG', q, cfg) == [(-4, 3)]                          # A: overlap 3 = minoverlap
    assert MM.alignments(b'TTTTTAC', q, dict(cfg, maxerrors=0)) == []              # ... 2: never visited
    assert MM.alignments(b'GCATTTT', q, dict(cfg, maxerrors=0)) == [(5, 3)]        # B
    assert MM.alignments(b'TTGCA', q, dict(cfg, maxerrors=0)) == [(3, 5), (3, 5)]  # B, then the read inside the sequence: twice
    assert MM.alignments(b'GCA', q, dict(cfg, maxerrors=0)) == [(5, 3)]            # rl == minoverlap: the last loop alone
    assert MM.alignments(b'TT' + q + b'T', q, dict(cfg, maxerrors=0)) == [(-2, 8)]
    assert MM.alignments(q, q, dict(cfg, maxerrors=0)) == [(0, 8)]
    assert MM.alignments(b'AgGTTGCA', q, cfg) == [(0, 8)] and MM.alignments(b'AgGTTGCa', q, cfg) == []
    assert MM.hit_bytes(b'TTTTACG', -4, 3) == b'ACG' and MM.hit_bytes(b'GCATTTT', 5, 3) == b'GCA'


@pytest.mark.parametrize('name', MM.CELLS)
def test_the_statement_finds_on_every_spec_what_was_planned(name):
    w = MM.cell(name)
    amin = ord(w.cfg['Amin'])
    for s in w.specs:
        start, ln = TM.trim(s.scores, amin)
        assert (start, ln) == (s.lead, len(s.read)), s
        read = s.bases[start:start + ln]
        got = MM.alignments(read, w.seqs[s.target], w.cfg)
        assert got == s.plan and bool(got) == s.hit, (s, got)
        assert len(s.offs) == (0 if s.geom.endswith('mo-1') else w.e if s.hit else w.e + 1), s
        if s.plan:                                                # the planned alignment holds exactly these mismatches
            p, L = s.plan[0]
            assert L == s.L, s
            hb, q = MM.hit_bytes(read, p, L), w.seqs[s.target][max(0, p):max(0, p) + L]
            assert [i for i in range(L) if hb[i] != q[i]] == list(s.offs), s
    # the record's name gives back the spec
    for bg, text in w.texts.items():
        raw = text.data.tobytes()
        for s in w.specs[::37] + w.specs[-1:]:
            at = text.starts[s.n]
            assert raw[at:raw.index(b'\n', at)].split(b' ')[0] == b'@M%s.%d' % (name.encode(), s.n)
            assert raw[text.reads[s.n]:text.reads[s.n] + len(s.read)] == s.read and text.spec_at(text.reads[s.n]) == s.n
        assert text.specs == w.specs and text.spec_at(0) is None and text.spec_at(text.nbytes - 1) is None


@pytest.mark.parametrize('name', MM.CELLS)
def test_every_cell_holds_every_geometry_seam_class_and_byte_kind(name):
    w = MM.cell(name)
    geoms = set(s.geom for s in w.specs)
    assert geoms == set(GEOMETRIES), geoms ^ set(GEOMETRIES)
    seams = MM.seam_classes(w.overlaps)
    want = ['first', 'last', 'm8-', 'm8', 'm16-', 'm16', 'rb0', 'rb1', 'dbl-', 'dbl', 'dword', 'lastdword']
    if name != 'S':                                                # (its overlaps end at 33 bytes)
        want += ['m64-', 'm64', 'm128-', 'm128']
    assert sorted(seams) == sorted(want)
    # every general geometry x seam class x byte kind, as a hit and as its twin with one mismatch more
    have = set((s.geom, s.seam, s.kind, s.hit) for s in w.specs)
    missing = [c for c in itertools.product(MM.GENERAL, seams, MM.KINDS, (True, False)) if c not in have]
    assert not missing, missing[:5]
    # half the specs of each seam class expect no hit
    for seam in seams:
        of = [s.hit for s in w.specs if s.seam == seam]
        assert len(of) >= 18 and 2 * sum(of) == len(of), seam
    # every multiple class at several overlap lengths
    for seam in seams:
        assert len(set(s.L for s in w.specs if s.seam == seam)) >= 5, seam
    # the bytes written: another base; N and '.' for a G and lower-case letters; 0x80 | base and 0xFF
    wrote = set(b for s in w.specs for b in s.wrote)
    assert wrote >= set(b'ACGTN.acgt') | {0xFF} | set(0x80 | b for b in b'ACGT'), sorted(wrote)
    # ... and on the seam itself every kind, for every seam class (the place's mismatch is of the spec's kind)
    for seam in seams:
        assert set(s.kind for s in w.specs if s.seam == seam) == set(MM.KINDS), seam
    # code-keeping copies of whole sequences: e substitutions in e seed blocks (a hit), e + 1 (none)
    keep = [s for s in w.specs if s.geom.startswith('keep-')]
    assert len(keep) >= 12 and sum(s.hit for s in keep) * 2 == len(keep)
    code = lambda b: {'A': 0, 'C': 1, 'G': 2, 'T': 3, 'N': 2, '.': 2}[chr(b).upper()]
    for s in keep:
        q = w.seqs[s.target]
        body = s.read[s.ro:s.ro + len(q)]
        assert body != q and [code(a) for a in body] == [code(b) for b in q], s
        assert len(set(o // w.pitch for o in s.offs)) == len(s.offs) and all(o % w.pitch < w.kseed and o // w.pitch <= w.e for o in s.offs), s
    # the sequences the seed index refuses are aimed at, and so are 4095 and 4096 bases
    aimed = set(s.target for s in w.specs if s.hit)
    assert aimed >= set(w.refused) | {w.nr[4095]}, (aimed, w.refused)


@pytest.mark.parametrize('name,bg', TEXTS, ids=lambda v: str(v))
def test_the_oracle_finds_on_every_spec_what_the_statement_does(name, bg):
    w = MM.cell(name)
    text, o = w.texts[bg], oracle_of(name, bg)
    got, want = text.by_spec(o['hits']), text.planned(len(w.seqs))
    for i, s in enumerate(text.specs):                             # every spec: none is left out because the oracle disagrees
        assert got.get(i, []) == want.get(i, []), (s, got.get(i))
    assert o['stats']['records_parsed'] > len(w.specs)


@pytest.mark.parametrize('name,bg', TEXTS, ids=lambda v: str(v))
def test_the_fold_of_the_statements_hits_is_the_oracles(name, bg):
    """coverage and mutations rebuilt hit by hit (analyse.py:57-78; the classes: A, C, G, T, N, anything else) from the
    statement's hits of the spec records on their targets and the oracle's other hits"""
    w = MM.cell(name)
    text, o = w.texts[bg], oracle_of(name, bg)
    off = [0]
    for q in w.seqs:
        off.append(off[-1] + len(q))
    cov, mut = [0] * off[-1], [0] * (6 * off[-1])

    def apply_hit(seq_nr, seq_pos, length, hitseq):
        seq = w.seqs[seq_nr]
        start = max(0, seq_pos)
        for i, j in enumerate(range(start, start + length)):
            cov[off[seq_nr] + j] += 1
            if hitseq[i] != seq[j]:
                mut[6 * (off[seq_nr] + j) + {65: 0, 67: 1, 71: 2, 84: 3, 78: 4}.get(hitseq[i], 5)] += 1
    others = 0
    for h, hs in zip(o['hits'], o['hitseqs']):
        i = text.spec_at(h.file_pos)
        if i is None or h.seq_nr != text.specs[i].target:
            apply_hit(h.seq_nr, h.seq_pos, h.length, hs); others += 1
    for s in w.specs:
        for p, ln in s.plan:
            apply_hit(s.target, p, ln, MM.hit_bytes(s.read, p, ln))
    assert others + sum(len(s.plan) for s in w.specs) == len(o['hits'])
    assert cov == o['coverage'] and mut == o['mutations']
    # classes 4 and 5 are in it: N, and '.', lower case and the high bytes
    assert sum(mut[4::6]) > 0 and sum(mut[5::6]) > 0


# ---- the long texts of the redo route ---------------------------------------------------------------------------

def test_the_long_text_holds_what_the_redo_route_is_to_meet():
    w = MM.cell('P')
    text, co = MM.long_text()
    longs = [(i, s) for i, s in enumerate(text.specs) if s.long]
    assert len(longs) == text.n_long and all(len(s.read) >= MM.KVQ_LONG_READ for _, s in longs) and text.n_long <= MM.KVQ_LONG_CAP
    assert sum(1 for s in text.specs if not s.long) == text.n_short >= 200 and all(len(s.read) < MM.KVQ_LONG_READ for s in text.specs if not s.long)
    for i, s in longs:
        assert TM.trim(s.scores, ord('.')) == (0, len(s.read)) and MM.alignments(s.read, w.seqs[s.target], w.cfg) == s.plan, s
        assert text.reads[i] % 4 == s.shift
    # the staged read on both sides of the LDS buffer's bound, every byte shift on each; a hit at the head and one flush with the tail
    lds = [(len(s.read) + text.reads[i] % 4, text.reads[i] % 4, s) for i, s in longs if s.geom == 'lds']
    for side in (True, False):
        assert len([1 for n, sh, s in lds if (n <= MM.KVQ_LONG_LDS) == side]) >= 6
        assert set(sh for n, sh, s in lds if (n <= MM.KVQ_LONG_LDS) == side) == {0, 1, 2, 3}
    assert {MM.KVQ_LONG_LDS, MM.KVQ_LONG_LDS + 1} <= set(n for n, sh, s in lds)
    assert all([p for p, ln in s.plan] == [0, -(len(s.read) - ln)] for n, sh, s in lds for p, ln in s.plan[:1])
    # every other geometry as a hit and as its twin, at every byte shift; hits that end on the read's last byte
    for geom in ('A@tail', 'B@head', 'Cr@head', 'Cr@tail', 'Cr@inside'):
        of = [(s.hit, text.reads[i] % 4) for i, s in longs if s.geom == geom]
        assert set(h for h, sh in of) == {True, False} and set(sh for h, sh in of) == {0, 1, 2, 3}, geom
    assert sum(1 for i, s in longs if s.plan and -s.plan[-1][0] + s.plan[-1][1] == len(s.read)) >= 20
    # the prefilter: all mismatches inside the first eight bases of the sequence
    pre = [s for i, s in longs if s.seam is None and s.geom != 'lds']
    assert all(max(s.offs) < 8 for s in pre) and sum(s.hit for s in pre) >= 4 and sum(not s.hit for s in pre) >= 4
    assert set(s.seam for i, s in longs) >= set(MM.seam_classes(w.overlaps))
    # every overlap length of the list at the read's tail (A) and at its head (B), as a hit and as its twin
    for geom in ('A@tail', 'B@head'):
        for hit in (True, False):
            assert set(s.L for i, s in longs if s.geom == geom and s.hit == hit) >= set(w.overlaps), (geom, hit)
    # the short records (kvq_match_all behind the redo): hits and their twins with one mismatch more in pairs, so that the
    # matcher is asked to reject at every seam class as often as to accept
    shorts = [s for s in text.specs if not s.long]
    seams = set(MM.seam_classes(w.overlaps))
    assert abs(sum(s.hit for s in shorts) - sum(not s.hit for s in shorts)) <= 4
    assert set(s.seam for s in shorts if s.hit) >= seams and set(s.seam for s in shorts if not s.hit and s.offs) >= seams
    assert set(s.kind for s in shorts if not s.hit and s.offs) == set(MM.KINDS)
    # every chunk behind the head: one spec record that starts inside the first tile and ends beyond that tile's look-ahead (the
    # tile leaves it alone), or one tile with more newlines than its table holds (it leaves every record)
    raw = text.data.tobytes()
    left = 0
    for a, b in zip(co[1:-1], co[2:]):
        a, b = int(a), int(b)
        inside = [i for i in range(len(text.specs)) if a <= text.starts[i] < b]
        if text.specs[inside[0]].geom == 'lds':
            i, = inside
            assert text.starts[i] - a < MM.TILE_OWNS - 160 and text.ends[i] - a > MM.TILE_OWNS + MM.LOOKAHEAD + 160
            left += 1
        else:
            assert b - a < MM.TILE_OWNS - 16 and raw.count(b'\n', a, b) > MM.BP_NLCAP
            left += raw.count(b'\n', a, b) // 4
    assert left == text.n_left <= MM.KVQ_REDO_RECORDS
    o = O.scan_memory(text.data, w.seqs_kept, fold=True, nthreads=16, **w.cfg)
    got, want = text.by_spec(o['hits']), text.planned(len(w.seqs_kept))
    for i, s in enumerate(text.specs):
        assert got.get(i, []) == want.get(i, []), (s, got.get(i))


def test_the_text_of_one_long_read_too_many():
    """KVQ_LONG_CAP + 1 reads of 1024 bases made of the repeat that eight sequences of the table begin with"""
    w = MM.cell('P')
    text, n = MM.cap_text()
    seqs = w.flood_table()
    assert n == MM.KVQ_LONG_CAP + 1 and seqs[:len(w.seqs_kept)] == w.seqs_kept
    raw = text.data.tobytes()
    lines = raw.split(b'\n')[1::4]
    assert sum(1 for ln in lines if len(ln) == 1024) == n and max(len(ln) for ln in lines) == 1024
    # every one of them has far more candidates than a wave's queue holds (96): at the positions the seed filter looks at
    # (multiples of the index stride) stands an 8-mer of the repeat, and each of its eight phases is a seed of the table
    seeds = set(q[w.pitch * j + sft:w.pitch * j + sft + 8] for q in seqs[len(w.seqs_kept):] for j in range(w.e + 1) for sft in range(w.stride))
    assert seeds == set((MM.FLOOD_UNIT * 2)[ph:ph + 8] for ph in range(8))
    for ln in lines:
        if len(ln) == 1024:
            assert sum(1 for p in range(0, 1024 - 8, w.stride) if ln[p:p + 8] in seeds) > 3 * 96
    o = O.scan_memory(text.data, seqs, fold=True, nthreads=16, **w.cfg)
    got, want = text.by_spec(o['hits']), text.planned(len(seqs))
    assert len(want) > 100 and sum(1 for s in text.specs if not s.hit) > 100
    assert set(s.geom for s in text.specs) == {'Cr@head', 'Cr@tail', 'Cr@inside'} and set(s.kind for s in text.specs) == set(MM.KINDS)
    for i, s in enumerate(text.specs):
        assert MM.alignments(s.read, seqs[s.target], w.cfg) == s.plan, s
        assert got.get(i, []) == want.get(i, []), (s, got.get(i))


def test_the_text_whose_tiles_leave_more_records_than_the_redo_takes():
    w = MM.cell('P')
    text, co, n = MM.overflow_text()
    raw = text.data.tobytes()
    lines = raw[int(co[1]):].split(b'\n')[1::4]
    assert sum(1 for ln in lines if len(ln) == 1024) == n and sum(1 for ln in lines if len(ln) > 1024) == 0
    # seventeen a chunk of one tile that overflows its newline table: more records than the redo's list holds
    for a, b in zip(co[1:-1], co[2:]):
        assert b - a < MM.TILE_OWNS - 16 and raw.count(b'\n', int(a), int(b)) > MM.BP_NLCAP
    assert len(lines) == text.n_left > MM.KVQ_REDO_RECORDS
    o = O.scan_memory(text.data, w.seqs_kept, fold=True, nthreads=16, **w.cfg)
    got, want = text.by_spec(o['hits']), text.planned(len(w.seqs_kept))
    assert len(want) > 100
    for i, s in enumerate(text.specs):
        assert MM.alignments(s.read, w.seqs[s.target], w.cfg) == s.plan, s
        assert got.get(i, []) == want.get(i, []), (s, got.get(i))
