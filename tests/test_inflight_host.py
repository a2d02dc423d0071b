"""
What tests/inflight.py builds for tests/test_gpu_inflight.py, checked without a GPU: the generators' properties against
the oracle, and the plain statement of kvq_verify_survivors' round loop against its misstatements.
"""
import ctypes as C
import re

import numpy as np
import pytest

import inflight as F
import kernel_matrix as KM
from kvarq_amd import _lib, scan


def test_nine_answers_that_differ_pairwise():
    """three tables x three texts: 100 hits and more each, and no two of the nine agree in their hits or in any counter array --
    a scan that used another scan object's table, text, list, arena or counters cannot give the expected answer by luck"""
    fam = F.families()
    assert len(fam) == 9
    for key, o in fam.items():
        assert len(o['hits']) >= 100, (key, len(o['hits']))
    keys = sorted(fam)
    for i, x in enumerate(keys):
        for y in keys[i + 1:]:
            a, b = fam[x], fam[y]
            assert tuple(a['hits']) != tuple(b['hits']) and a['hitseqs'] != b['hitseqs'], (x, y)
            for name in ('nseqhits', 'nseqbasehits'):
                assert a['stats'][name] != b['stats'][name], (x, y, name)
            # (the read lengths and the record count belong to the text, whatever the table)
            assert (a['stats']['readlengths'] != b['stats']['readlengths'] and a['stats']['records_parsed'] != b['stats']['records_parsed']) or x[1] == y[1], (x, y)
            assert a['coverage'] != b['coverage'] and a['mutations'] != b['mutations'], (x, y)
    # the texts differ in size, tiles and chunks; each can be cut in two batches, and one at least off a 16-byte boundary
    tiles = [sum(KM.tiles_of(t)[1]) for t in F.texts()]
    assert len(set(tiles)) == 3 and len(set(t.nbytes for t in F.texts())) == 3, tiles
    cuts = [F.two_batches(t, scan.chunk_offsets(t)) for t in F.texts()]
    for t, two in zip(F.texts(), cuts):
        (b0, n0, co0, f0), (b1, n1, co1, f1) = two
        assert b0 == 0 and b1 % 16 == 0 and f1 == b1 and b1 + n1 == t.nbytes and n0 == b1 + int(co1[0])
        assert len(co0) >= 2 and len(co1) >= 2
    assert any(int(two[1][2][0]) for two in cuts), 'every cut lies on a 16-byte boundary'
    # the tables: three seed lengths or kernel families are not promised, three configurations' worth of different sequences are
    names = [n for n, _, _ in F.tables()]
    assert names == ['mtbc', 'spoligo', 'loose']
    assert KM.seed_k(F.tables()[0][2]) == 8 and KM.seed_k(F.tables()[2][2]) == 7
    assert F.tables()[2][2]['maxerrors'] != F.tables()[0][2]['maxerrors'] and F.tables()[2][2]['minoverlap'] != F.tables()[0][2]['minoverlap']


def test_the_dense_text_is_dense():
    """more than three hits a read: every read lies on a template's locus"""
    _, seqs, cfg = F.tables()[0]
    o = F.oracle_of(F.dense_text(), seqs, cfg)
    assert o['stats']['records_parsed'] == F.DENSE_RECORDS and len(o['hits']) > 3 * F.DENSE_RECORDS
    with_hit = len(set(h.file_pos for h in o['hits']))
    assert with_hit > 0.97 * F.DENSE_RECORDS, with_hit


def test_the_draw_order_of_one_workgroup():
    """draw_order against what the kernel's text says by hand: 28 tiles leave every share with one tile or none, and the shares are
    tried in the order 37 i mod 64 from the one the workgroup is in; with ten tiles a share the shares come in the order 37 k mod 64,
    each from its first tile to its last.  Never the order of the text"""
    assert F.draw_order(28) == [20, 8, 24, 5, 21, 2, 18, 27, 15, 3, 12, 0, 9, 25, 6, 22, 10, 19, 7, 16, 4, 13, 1, 17, 26, 14, 23, 11]
    assert F.draw_order(640) == [10 * (37 * k % 64) + j for k in range(64) for j in range(10)]
    for n in (0, 1, 2, 3, 29, 63, 64, 65, 127, 128, 272, 1000):
        order = F.draw_order(n)
        assert sorted(order) == list(range(n)), n
        # inside a share the tiles come in their order, and a share is finished before the next is begun
        share = [next(sh for sh in range(64) if sh * n // 64 <= g < (sh + 1) * n // 64) for g in order]
        firsts = [sh for k, sh in enumerate(share) if k == 0 or share[k - 1] != sh]
        assert len(firsts) == len(set(firsts)) and all(a < b for a, b, x, y in zip(order, order[1:], share, share[1:]) if x == y), n
    assert F.draw_order(28) != list(range(28)) and F.draw_order(640) != list(range(640))


def test_the_silent_stretch_yields_no_hit_of_its_own():
    _, seqs, cfg = F.tables()[0]
    text, cls, alone, order = F.silent_text()
    spans = F.tile_spans(text)
    assert list(order) == F.draw_order(len(spans)) and KM.tiles_of(text)[0] == 39760 and len(spans) == sum(KM.tiles_of(text)[1])
    # the classes of the tiles in the order the workgroup takes them: true hits, near-misses, true hits -- each run unbroken
    of_tile = []
    for a, b in spans:
        inside = set(int(cls[r]) for r in range(-(-a // F.RB), b // F.RB))
        assert len(inside) == 1 and F.NEUTRAL not in inside, (a, b, inside)
        of_tile.append(inside.pop())
    drawn = [of_tile[g] for g in order]
    h, st = F.SILENT_HEAD_TILES, F.SILENT_STRETCH_TILES
    assert drawn == [F.HEAD] * h + [F.STRETCH] * st + [F.TAIL] * (len(order) - h - st) and len(order) - h - st >= 4
    assert [of_tile[g] for g in range(len(spans))] != sorted(of_tile)            # (in the text they are interleaved)
    # every record that does not lie wholly inside one tile is neutral, and no other
    for r in range(len(cls)):
        whole = any(a <= r * F.RB and (r + 1) * F.RB <= b for a, b in spans)
        assert whole == (cls[r] != F.NEUTRAL), r
    o = F.oracle_of(text, seqs, cfg)
    rec = np.array([h_.file_pos // F.RB for h_ in o['hits']])
    assert len(set(rec.tolist())) == len(rec)                                       # (a hit a read: the template on its strand)
    assert sorted(rec.tolist()) == np.nonzero((cls == F.HEAD) | (cls == F.TAIL))[0].tolist()
    assert len(F.oracle_of(alone, seqs, cfg)['hits']) == 0
    assert alone.nbytes == int((cls == F.STRETCH).sum()) * F.RB
    # every read of the stretch has exactly maxerrors + 1 mismatches against its template on one strand, on the one
    # diagonal that holds the template whole (the statement of the four loops: tests/match_matrix.py)
    import match_matrix as MM
    recs = text.reshape(-1, F.RB)[cls == F.STRETCH]
    for rec_ in recs[::97]:
        read = rec_[21:21 + F.L].tobytes()
        best = min(int(np.count_nonzero(np.frombuffer(read[i:i + 51], dtype=np.uint8) != np.frombuffer(q, dtype=np.uint8)))
                   for q in list(seqs[:27]) + list(seqs[132:159]) for i in range(F.L - 50))
        assert best == cfg['maxerrors'] + 1, best
        assert not any(MM.alignments(read, q, cfg) for q in list(seqs[:27]) + list(seqs[132:159]))


# (n, grid, block): what the GPU tests walk.  The slot counts are the ones an MI355X gave (profiles/inflight_tests.txt; they move
# by a few chunks from run to run: which wave had which chunk open); 100 is the list cut by KVQ_SURV_CAP
WALKED = [(n, grid, 256) for grid in (64, 3, 1) for n in F.MEASURED_SLOTS + (100,)] + [(n, 256, 1024) for n in F.MEASURED_SLOTS]
EDGES = [(0, 3, 256), (1, 3, 256), (255, 1, 256), (256, 1, 256), (257, 1, 256), (768, 3, 256), (769, 3, 256), (16384, 64, 256), (32768, 64, 256), (32784, 64, 256)]


@pytest.mark.parametrize('n,grid,block', WALKED + EDGES)
def test_the_round_walk_visits_every_slot_once(n, grid, block):
    walk = F.round_walk(n, grid, block)
    assert F.walk_is_exact(walk, n, grid, block)
    # the rounds are the same for every thread of a workgroup (the barriers inside are uniform), a round covers a block
    for wg, rounds in walk.items():
        for k, r in enumerate(rounds):
            assert r and r[0] == (wg + k * grid) * block and r == list(range(r[0], min(r[0] + block, n)))
    most, fewest = F.rounds_per_workgroup(n, grid, block)
    assert most == -(-n // (grid * block)) and most - fewest <= 1


def test_the_wrong_walks_are_told_apart():
    """a step of blockDim alone visits slots twice, base = blockIdx.x overlaps the workgroups, <= on the slot reads one past
    the list, <= on the loop walks a round too many where a workgroup's base lands on n"""
    caught = dict((w, 0) for w in F.WRONG_WALKS)
    for n, grid, block in WALKED + EDGES:
        for w in F.WRONG_WALKS:
            if w == 'step' and n * grid > 4000000:
                continue                                    # (every workgroup would walk the whole list: the smaller lists tell as much)
            if not F.walk_is_exact(F.round_walk(n, grid, block, wrong=w), n, grid, block):
                caught[w] += 1
    # what the GPU tests walk with more than one workgroup tells the first two apart, every list that does not end on a block the third
    for n, g, b in WALKED:
        if g > 1 and n > g:
            assert not F.walk_is_exact(F.round_walk(n, g, b, wrong='first'), n, g, b), (n, g, b)
            assert n <= b or n * g > 4000000 or not F.walk_is_exact(F.round_walk(n, g, b, wrong='step'), n, g, b), (n, g, b)
        if n % b:
            assert not F.walk_is_exact(F.round_walk(n, g, b, wrong='slot<='), n, g, b), (n, g, b)
    assert all(caught[w] >= 3 for w in F.WRONG_WALKS), caught
    # (one workgroup: its step IS the block, and 0 * block is 0 -- those two misstatements are no misstatements there)
    assert F.walk_is_exact(F.round_walk(1000, 1, 256, wrong='step'), 1000, 1, 256)


def test_the_arithmetic_of_the_silent_rounds():
    # two silent rounds need 11 rounds' worth of range (one lost to the range's ends, eight to open chunks): 11 * 256 + 2 * 8 * 16 slots
    assert F.silent_rounds(0) == 0 - F.OPEN_CHUNKS and F.silent_rounds(3072 - 1) < 2 <= F.silent_rounds(3072)
    assert F.silent_rounds(F.MEASURED_ALONE_SLOTS) >= 2


def test_launch_info_is_declared_as_it_is_documented():
    """(a scan object cannot be made without a device: that the report is all zeros before the first launch, after a reset and
    for an exhaustive scan is asserted on the GPU, tests/test_gpu_inflight.py)"""
    assert _lib.PROTOTYPES['kvq_scan_launch_info'] == (None, [C.c_void_p, C.POINTER(C.c_int64)])
    assert len(scan.Scanner.LAUNCH_INFO) == 10 and len(scan.Scanner.GRID_CAP_KINDS) == 4
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kvarq_hip.h')) as f:
        head = f.read()
    assert re.search(r'void\s+kvq_scan_launch_info\(const kvq_scan \*s, int64_t out\[10\]\);', head)
