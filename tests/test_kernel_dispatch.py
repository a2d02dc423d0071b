"""
CPU-only checks of which instantiation of the seed-filter scan kernel (kvq_scan_bp) the launcher picks for a
batch -- kvq_scan_kernel_pick is the very function kvq_seeded_launch calls -- at every boundary of its inputs, of
the tile the head of a text gives (kvq_tile_for_text), and of the workloads tests/test_gpu_kernel_matrix.py runs on
the GPU: each lands on its cell and gives the oracle hits in every planted class it aims at.
"""
import bisect
import ctypes as C
import os

import numpy as np
import pytest

import kernel_matrix as KM
from kvarq_amd import _lib, synth
from oracle import oracle as O

# kernels_seeded.hip: bytes a tile owns at the full look-ahead, the look-ahead, the least a tile owns, the newline block
ST_TILE, ST_OV, ST_TILE_MIN, ST_BLK, ST_THREADS = 36640, 4160, 30960, 80, 512
TILE = ST_TILE + ST_OV - 1040          # the tile of reads up to 190 bases (the shortest look-ahead)


def pick(k=8, stride=2, dense=False, rec_bytes=0, tile=TILE, dbg=0):
    return _lib.kernel_cell(_lib.lib().kvq_scan_kernel_pick(k, stride, 1 if dense else 0, rec_bytes, tile, dbg))


def tile_for_text(text):
    rb = C.c_uint32()
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = min(arr.nbytes, 128 << 10)
    tile = _lib.lib().kvq_tile_for_text(arr.ctypes.data, n, C.byref(rb))
    return tile, rb.value


def choose_tile(maxline, rec_bytes):
    """kvq_choose_tile, restated"""
    if maxline == 0:
        return ST_TILE
    ov = (4 * (maxline + 2) + 160 + ST_BLK - 1) // ST_BLK * ST_BLK
    ov = max(1040, min(ov, ST_OV))
    tile = ST_TILE + ST_OV - ov
    if rec_bytes >= 40:
        n_full = tile // rec_bytes + 1
        p = 1
        while 2 * p <= n_full:
            p *= 2
        if 16 <= p <= ST_THREADS and n_full > p:
            cut = (p - 1) * rec_bytes // ST_BLK * ST_BLK
            if cut >= ST_TILE_MIN and cut * 100 >= tile * 78:
                tile = cut
    return tile


def rec_for(n_full, tile=TILE):
    """a record size that lets a tile own exactly n_full records"""
    r = next(r for r in range(tile // (n_full - 1), 0, -1) if tile // r + 1 >= n_full)
    assert tile // r + 1 == n_full
    return r


@pytest.mark.parametrize('n_full,lg', [(32, -1), (33, 3), (64, 3), (65, 2), (128, 2), (129, 1), (256, 1), (257, -1), (1000, -1)])
def test_lane_group_at_every_records_per_tile_boundary(n_full, lg):
    # both ends of the tiles that own exactly n_full records of a size
    for rb in (40, 41, 155, 325, 625, 1225):
        for tile in (rb * (n_full - 1), rb * n_full - 1):
            assert pick(rec_bytes=rb, tile=tile) == dict(k=8, stride=2, lg=lg, dense=False), (n_full, tile, rb)
            # seeds shorter than 8 and dense tables have the general kernel and the four-lane one only
            for k, dense in ((5, False), (6, True), (7, False), (8, True)):
                assert pick(k=k, dense=dense, rec_bytes=rb, tile=tile) == dict(k=k, stride=2, lg=lg if lg == 2 else -1, dense=True)


def test_records_below_40_bytes_or_unknown_take_the_general_kernel():
    assert pick(rec_bytes=40, tile=40 * 100) == dict(k=8, stride=2, lg=2, dense=False)
    assert pick(rec_bytes=39, tile=39 * 100) == dict(k=8, stride=2, lg=-1, dense=False)
    assert pick(rec_bytes=0) == dict(k=8, stride=2, lg=-1, dense=False)


def test_stride_seed_length_and_family_of_the_cell():
    rb = rec_for(100)
    for stride in (2, 4, 8):
        for k in (5, 6, 7, 8):
            for dense in (False, True):
                got = pick(k=k, stride=stride, dense=dense, rec_bytes=rb)
                assert got == dict(k=k, stride=stride, lg=2, dense=dense or k < 8)
    # no instantiation for other strides or seed lengths
    L = _lib.lib()
    for k, stride in ((8, 1), (8, 3), (8, 16), (4, 2), (9, 2), (0, 8)):
        assert L.kvq_scan_kernel_pick(k, stride, 0, rb, TILE, 0) == -1


def test_diagnostic_switches_pick_the_builds_that_honour_them():
    L = _lib.lib()
    for n_full, lg in ((40, 3), (100, 2), (200, 1)):
        rb = rec_for(n_full)
        plain = L.kvq_scan_kernel_pick(8, 4, 0, rb, TILE, 0)
        assert not plain & (_lib.CELL_DIAG | _lib.CELL_STAMPS)
        # any KVQ_DBG bit but the stamps: the general kernel or the four-lane one, with the diagnostics
        diag = L.kvq_scan_kernel_pick(8, 4, 0, rb, TILE, 1)
        assert diag & _lib.CELL_DIAG and _lib.kernel_cell(diag)['lg'] == (2 if lg == 2 else -1)
        # the stamps (bit 16): the instrumented builds of those two, halving, even on a dense table
        st = L.kvq_scan_kernel_pick(8, 4, 1, rb, TILE, 16)
        assert st & _lib.CELL_STAMPS and not st & (_lib.CELL_DIAG | _lib.CELL_DENSE)
        assert _lib.kernel_cell(st)['lg'] == (2 if lg == 2 else -1)
    # the K < 8 and the draining kernels are diagnostic builds already
    assert L.kvq_scan_kernel_pick(6, 2, 0, rec_for(100), TILE, 0) & _lib.CELL_DIAG
    assert L.kvq_scan_kernel_pick(8, 2, 1, rec_for(100), TILE, 0) & _lib.CELL_DIAG


@pytest.fixture(scope='module')
def g():
    return synth.genome()


# (kvq_choose_tile cuts a tile to a whole number of lane groups where it can: 50-base reads land on two lanes a read,
# 125 on four, 250 on eight)
@pytest.mark.parametrize('L,lg', [(40, -1), (48, -1), (50, 1), (64, 1), (75, 1), (110, 1), (125, 2), (150, 2), (250, 3),
                                  (300, 3), (550, -1), (600, -1), (1000, -1)])
def test_tile_and_lane_group_of_uniform_reads(g, L, lg):
    if os.environ.get('KVQ_TILE'):
        pytest.skip('KVQ_TILE sets the tile')
    n = (160 << 10) // synth.record_bytes(L) + 2
    text = synth.reads(g, 5, n, L)
    tile, rb = tile_for_text(text)
    head = text[:128 << 10].tobytes()
    lines = head.count(b'\n')
    whole = head.rindex(b'\n') + 1
    assert rb == whole * 4 // lines and abs(rb - synth.record_bytes(L)) <= synth.record_bytes(L) // 8
    assert tile == choose_tile(L + 1, rb)
    assert pick(rec_bytes=rb, tile=tile)['lg'] == lg


def test_the_tile_is_chosen_from_the_head_of_the_text_alone(g):
    if os.environ.get('KVQ_TILE'):
        pytest.skip('KVQ_TILE sets the tile')
    for head_len, body_len in ((150, 50), (150, 300), (75, 40), (300, 600), (50, 150)):
        nh = (130 << 10) // synth.record_bytes(head_len) + 1
        head = synth.reads(g, 0, nh, head_len)
        body = synth.reads(g, nh, 4000, body_len)
        text = np.concatenate([head, body])
        assert tile_for_text(text) == tile_for_text(head)
        assert tile_for_text(text) != tile_for_text(body)
    # the longest line of the head sets the look-ahead: one 3000-base read among 150-base ones takes the full one
    rb = synth.record_bytes(150)
    head = synth.reads(g, 0, 200, 150).tobytes()
    long_rec = b'@long\n' + b'A' * 3000 + b'\n+\n' + b'I' * 3000 + b'\n'
    text = head[:100 * rb] + long_rec + head[100 * rb:]
    tile, rbytes = tile_for_text(text)
    assert tile == choose_tile(3001, rbytes) and tile < TILE
    # fewer than 16 lines: nothing known about the records
    tile, rbytes = tile_for_text(head[:3 * rb])
    assert rbytes == 0 and tile == choose_tile(151, 0)


@pytest.mark.parametrize('cell', KM.CELLS, ids=KM.cell_id)
def test_each_cell_workload_lands_on_its_cell_and_is_not_vacuous(g, cell):
    """the GPU matrix is only as good as its workloads: each must land on its cell (stride and density of its table,
    lane group of its text), and give the oracle hits -- in every class of planted record that must hit, and none in
    those that must not"""
    w = KM.Workload(cell, g)
    k, stride, lg, dense = cell
    e = w.cfg['maxerrors']
    assert len(KM.CELLS) == 36 and len(set(KM.CELLS)) == 36
    assert KM.seed_k(w.cfg) == k and KM.index_stride(w.seqs, k, e) == stride
    if k == 8:
        assert KM.index_dense(w.seqs, k, e, stride) == dense
    assert not KM.seedable(w.plus[w.refused_n], k, e) and not KM.seedable(w.plus[w.refused_short], k, e)
    assert len(w.texts) == (2 if lg > 0 else 1)
    for i, text in enumerate(w.texts):
        tile, rb = tile_for_text(text)
        if not os.environ.get('KVQ_TILE'):
            assert pick(k, stride, dense, rb, tile) == dict(k=k, stride=stride, lg=lg, dense=dense), (i, tile, rb)
        starts, names = w.record_names(text)
        assert len(starts) >= 1000 and text.nbytes >= 20 * tile          # (many tiles, drawn by many workgroups)
        # (under KVQ_GRID=1 and 5 a workgroup walks all of them, or a fifth: tests/test_gpu_kernel_matrix.py)
        assert KM.tiles_of(text)[0] == tile and sum(KM.tiles_of(text)[1]) >= 25, (i, KM.tiles_of(text))
        o = O.scan_memory(text, w.seqs, fold=True, nthreads=min(16, os.cpu_count() or 1), **w.cfg)
        assert len(o['hits']) >= 100, (i, len(o['hits']))
        by = w.hits_by_class(text, o['hits'])
        for cls, (aim, want) in sorted(w.classes.items()):
            if want is True:
                assert by[cls] > 0, (i, cls)
            else:
                assert by[cls] == 0, (i, cls, by[cls])
        # the residue reads hold their sequence at read offset d = their residue modulo 8, on both strands
        res = [(names[bisect.bisect_right(starts, h.file_pos) - 1], h) for h in o['hits']]
        res = [(int(n[4:].split('.')[0]), h) for n, h in res if n.startswith('Pres') and h.seq_nr in w.classes[n[1:].split('.')[0]][0]]
        assert sorted(set(d for d, _ in res)) == list(range(8)) and all(-h.seq_pos % 8 == d for d, h in res), i
        # the refused sequences are met by the exhaustive kernels, the seeded ones by the seed filter
        hit_seqs = set(h.seq_nr % w.np for h in o['hits'])
        assert {w.refused_n, w.refused_short} <= hit_seqs and len(hit_seqs - {w.refused_n, w.refused_short}) > 5


def test_the_long_walk_reaches_what_it_is_for(g):
    """KM.long_walk() is only worth its time if a lone workgroup must flush its read-length histogram, every share of
    the tiles lets a workgroup stay for a while, and no tile runs out of its tables (a tile that does leaves its records
    to the redo chain, which proves nothing about the scan kernel)"""
    if os.environ.get('KVQ_TILE'):
        pytest.skip('KVQ_TILE sets the tile')
    w = KM.long_walk(g)
    text = w.text
    tile, per_chunk = KM.tiles_of(text)
    nt = sum(per_chunk)
    assert tile == choose_tile(w.ODD + 1, 2 * w.READ + 8) == TILE
    assert nt >= 256 and nt > 2 * KM.ST_HIST_TILES
    shares = [KM.shard_begin(sh + 1, nt) - KM.shard_begin(sh, nt) for sh in range(KM.BP_SHARDS)]
    assert sum(shares) == nt and min(shares) >= 4, shares
    # both configurations land on the kernel that works the lane group out per tile, and every sequence is seeded
    rb = tile_for_text(text)[1]
    for (k, stride, lg, dense), cfg in zip(w.CELLS, w.cfgs):
        assert pick(k, stride, dense, rb, tile) == dict(k=k, stride=stride, lg=lg, dense=dense)
        assert all(KM.seedable(q, k, cfg['maxerrors']) for q in w.seqs)
    # no stretch of a tile's bytes holds more record starts than a tile's tables, no window of a tile more newlines
    nl = np.flatnonzero(text == 10)
    starts = np.concatenate([[0], nl[3::4][:-1] + 1])
    assert len(nl) == 4 * w.n_reads and bool((text[starts] == ord('@')).all())
    per_tile = np.searchsorted(starts, starts + tile) - np.arange(len(starts))
    per_window = np.searchsorted(nl, nl + KM.BP_WINDOW) - np.arange(len(nl))
    assert 400 < per_tile.max() <= KM.ST_RCAP and 1800 < per_window.max() <= KM.BP_NLCAP, (per_tile.max(), per_window.max())
    # with the flush a bin stays below 2^16 between two flushes; without it a lone workgroup's bin of READ runs over
    # (129 tiles of 510 records, as the kernel's bound is stated: 129 * 510 > 65535 >= 100 * 512), and READ is even: the
    # carry goes into the bin of READ + 1 in the same word
    assert KM.ST_HIST_TILES * KM.ST_RCAP <= 65535 < 129 * 510
    assert KM.ST_HIST_TILES * int(per_tile.max()) <= 65535 < w.n_even and w.READ % 2 == 0 and w.ODD == w.READ + 1
    assert w.n_reads - w.n_even >= 1000 and w.n_planted >= 1000
    for cfg in w.cfgs:
        o = O.scan_memory(text, w.seqs, fold=True, nthreads=min(16, os.cpu_count() or 1), **cfg)
        rls = o['stats']['readlengths']
        assert len(rls) == w.ODD + 1 and rls[w.READ] == w.n_even and rls[w.ODD] == w.n_reads - w.n_even
        assert len(o['hits']) >= 1000
        # the hits are spread over the walk: every tenth of the text has some
        tenth = np.bincount([h.file_pos * 10 // text.nbytes for h in o['hits']], minlength=10)
        assert tenth.min() >= 50, tenth


def test_kvq_scan_grid_is_declared_and_bound():
    """r['grid'] is how the GPU tests see that KVQ_GRID was taken"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kvarq_hip.h')) as f:
        assert 'int32_t kvq_scan_grid(const kvq_scan *s);' in f.read()
    assert _lib.PROTOTYPES['kvq_scan_grid'] == _lib.PROTOTYPES['kvq_scan_kernel']
    assert _lib.lib().kvq_scan_grid.restype is C.c_int32
