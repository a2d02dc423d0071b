"""
Inputs for scans in flight: what kvq_seeded_launch does when the scan in front is still on the device.

Such a launch publishes the chain AHEAD of its kvq_verify_survivors (`beside`): the next scan object's persistent kernel
runs while this object's survivors, validation, redo, fold, record gathering, input passes and finish tail still do, and
the survivors are verified by 64 x 256 threads (KVQ_SV_GRID x 256) instead of 256 x 1024, so that a workgroup walks the
round loop of that kernel many times where it walked it once.  Three things are built here for it:

* ``families()``: three tables x three texts whose nine oracle answers differ pairwise in hits and in every counter
  array -- a kernel that read another scan object's list, arena, counters, fail word or pool would give a wrong answer,
  not the expected one;
* ``dense_text()``: reads sampled from the templates' own loci, every one a hit on several diagonals: thousands of
  survivors' slots per hundred tiles, for the rounds; ``crowded_text()``: a dozen hits a read, for the rounds of the large launch;
* ``silent_text()``: true hits, then a stretch of reads with exactly maxerrors + 1 mismatches (they pass the 16-base
  test of the scan kernel and fail the byte-exact one), then true hits -- in the order in which ONE scan workgroup takes
  the tiles (``draw_order``), which is not the order of the text: rounds of kvq_verify_survivors that emit nothing (its
  third barrier is skipped) between rounds that do.

``round_walk`` is the plain statement of the kernel's round loop, with the wrong statements beside it.

tests/test_inflight_host.py checks all of this against the oracle without a GPU; tests/test_gpu_inflight.py runs it
(children: tests/inflight_child.py) under KVQ_SV_MODE / KVQ_SV_GRID.  profiles/inflight_tests.txt is the census.
"""
import functools

import numpy as np

import cases
from kvarq_amd import synth

L = 150
RB = synth.record_bytes(L)
SV_CHUNK = 16                               # slots a wave takes at a time (KVQ_SURV_CHUNK)
SV_BLOCK_BESIDE, SV_BLOCK_BEHIND, SV_GRID_BESIDE, SV_GRID_BEHIND = 256, 1024, 64, 256      # kvq_seeded_launch
OPEN_CHUNKS = 8                             # waves of a scan workgroup: each holds one open chunk of the list

LOOSE = dict(maxerrors=3, minoverlap=28, minreadlength=28, Amin='.')


@functools.lru_cache(maxsize=None)
def genome():
    g = synth.genome()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def tables():
    """[(name, sequences, configuration)]: the MTBC-shaped table on both strands, the spoligo spacers, and the plus strands
    under four seeds of seven bases (maxerrors 3, minoverlap 28: the draining kernels, and the spacers -- shorter than
    the seed index takes -- through the exhaustive ones)"""
    g = genome()
    plus = synth.table(g)
    return (('mtbc', tuple(synth.both_strands(plus)), dict(cases.PRODUCT)),
            ('spoligo', tuple(s.encode() for s in synth.SPOLIGO_SPACERS), dict(cases.PRODUCT)),
            ('loose', tuple(plus), dict(LOOSE)))


def loci():
    """[(a, b)]: the genome intervals [a, b) the templates were cut from, 0-based; the direct-repeat locus as one"""
    out = [(p - 1 - synth.FLANK, p + synth.FLANK) for p, _ in synth.PHYLO_SNPS]
    out += [(p - 1 - synth.FLANK, p + synth.FLANK) for p, _, _ in synth.RESISTANCE_SNPS]
    out += [(a - 1 - synth.FLANK, b + synth.FLANK) for a, b in synth.RESISTANCE_REGIONS]
    dr = len(synth.SPOLIGO_SPACERS) * (len(synth.DIRECT_REPEAT) + 25)
    return out, (synth.DR_LOCUS - 1, synth.DR_LOCUS - 1 + dr)


_CODE = np.zeros(256, dtype=np.int64)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _i
_LETTERS = np.frombuffer(b'ACGT', dtype=np.uint8)


def records_of(bases, first=0):
    """(n, L) bases -> n records of synth's layout (21 bytes of name, the bases, '+', all scores 'I'), one uint8 array"""
    n = len(bases)
    out = np.empty((n, RB), dtype=np.uint8)
    out[:, :21] = np.frombuffer(b''.join((synth.HEADER_FMT % r).encode() for r in range(first, first + n)), dtype=np.uint8).reshape(n, 21)
    out[:, 21:21 + L] = bases
    out[:, 21 + L], out[:, 22 + L], out[:, 23 + L] = 10, ord('+'), 10
    out[:, 24 + L:24 + 2 * L] = synth.Q_GOOD
    out[:, 24 + 2 * L] = 10
    return out


def _cut(g, start, minus):
    """(n, L) bases: genome[start : start + L], reverse-complemented where `minus`"""
    jj = np.arange(L, dtype=np.int64)
    gi = np.where(minus[:, None], start[:, None] + (L - 1 - jj)[None, :], start[:, None] + jj[None, :])
    codes = _CODE[g[gi]]
    return np.where(minus[:, None], 3 - codes, codes)


def locus_reads(n, seed, first=0, dr_share=0.34, p_err=0.004):
    """n records whose reads overlap a template's locus by 40 bases or more, either strand, a substitution per 250 bases"""
    g = genome()
    rng = np.random.RandomState(seed)
    snp, dr = loci()
    snp = np.array(snp, dtype=np.int64)
    which = rng.randint(0, len(snp), n)
    a, b = snp[which, 0], snp[which, 1]
    in_dr = rng.random_sample(n) < dr_share
    a, b = np.where(in_dr, dr[0], a), np.where(in_dr, dr[1], b)
    lo, hi = a - L + 40, b - 40                                 # starts that leave 40 bases of overlap
    start = lo + (rng.random_sample(n) * (hi - lo + 1)).astype(np.int64)
    codes = _cut(g, start, rng.randint(0, 2, n).astype(bool))
    sub = rng.random_sample((n, L)) < p_err
    codes = np.where(sub, (codes + rng.randint(1, 4, (n, L))) % 4, codes)
    return records_of(_LETTERS[codes], first)


def mixed_text(n, dense_every, seed):
    """n records: synth's reads of the whole genome, every `dense_every`-th replaced by a read of a template's locus"""
    g = genome()
    out = synth.reads(g, seed * 1000003, n, L).reshape(n, RB).copy()
    at = np.arange(seed % dense_every, n, dense_every)
    out[at] = locus_reads(len(at), seed, first=seed * 1000003 + n).reshape(len(at), RB)
    return out.reshape(-1)


# (records, every how many a read of a locus, generator seed): 29, 44 and 68 tiles of 39 760 bytes, two or three chunks
TEXTS = ((3400, 6, 11), (5200, 9, 12), (8100, 5, 13))


@functools.lru_cache(maxsize=None)
def texts():
    out = []
    for n, every, seed in TEXTS:
        t = mixed_text(n, every, seed)
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


def oracle_of(text, seqs, cfg):
    from oracle import oracle as O
    return O.scan_memory(text, list(seqs), fold=True, nthreads=16, **cfg)


@functools.lru_cache(maxsize=None)
def families():
    """{(table, text): the oracle's answer}, nine of them"""
    return dict(((a, b), oracle_of(text, seqs, cfg)) for a, (_, seqs, cfg) in enumerate(tables()) for b, text in enumerate(texts()))


def two_batches(text, chunk_off):
    """[(base, nbytes, chunk offsets relative to base, fpos_base)]: the text as two device batches cut at a chunk offset, the second
    one's base pointer aligned down to 16 bytes -- the way bench.py cuts its own"""
    co = np.asarray(chunk_off, dtype=np.int64)
    assert len(co) >= 3, 'a text of one chunk cannot be cut'
    mid = (len(co) - 1) // 2
    out = []
    for i, j in ((0, mid), (mid, len(co) - 1)):
        base = int(co[i]) & ~15
        out.append((base, int(co[j]) - base, (co[i:j + 1] - base).copy(), base))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the dense text and the silent stretch
# ---------------------------------------------------------------------------------------------------------------

# what an MI355X gave (profiles/inflight_tests.txt): the slots of the lists of the dense, the silent and the crowded text, and of
# the silent stretch's records alone
MEASURED_SLOTS = (48875, 10053, 585123)
MEASURED_ALONE_SLOTS = 5031

DENSE_RECORDS = 4000                       # 33 tiles, a dozen slots a read: three rounds of 64 x 256 need 32 768 = 2 700 reads; the rest is margin
CROWD = (1472337, 1472362)                 # twelve resistance templates (and their other strands) lie within these 26 bases
CROWD_RECORDS = 15000                      # 39 slots a read on an MI355X: two rounds of 256 x 1024 cover 524 288


@functools.lru_cache(maxsize=None)
def dense_text(n=DENSE_RECORDS):
    t = locus_reads(n, 4242).reshape(-1)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def crowded_text(n=CROWD_RECORDS):
    """reads that hold all twelve templates of CROWD whole, on either strand: a dozen true hits a read, each found by half a dozen
    seeds -- the cheapest way to a list that 256 x 1024 threads walk in several rounds (more than 524 288 slots)"""
    g = genome()
    rng = np.random.RandomState(4343)
    lo, hi = CROWD[0] - 1 - synth.FLANK, CROWD[1] + synth.FLANK          # [lo, hi): the bases the templates cover
    start = rng.randint(hi - L, lo + 1, n).astype(np.int64)
    codes = _cut(g, start, rng.randint(0, 2, n).astype(bool))
    sub = rng.random_sample((n, L)) < 0.004
    codes = np.where(sub, (codes + rng.randint(1, 4, (n, L))) % 4, codes)
    t = records_of(_LETTERS[codes]).reshape(-1)
    t.setflags(write=False)
    return t


def snp_reads(n, seed, mismatches, first=0):
    """n records whose read holds one whole phylo-SNP template (51 bases; none of them has a neighbour within a read's length)
    with exactly `mismatches` substitutions against it, 1 <= mismatches <= 3: the SNP base itself -- the genome has the other
    allele --, and the rest side by side in ONE half of the template, 26 bases or more of it left whole.  Either strand, the
    template anywhere from 24 to 75 bases into the read, so that the read's own head and tail blocks lie outside it"""
    assert 1 <= mismatches <= 3
    g = genome()
    rng = np.random.RandomState(seed)
    pos = np.array([p for p, _ in synth.PHYLO_SNPS], dtype=np.int64)
    allele = _CODE[np.frombuffer(''.join(b for _, b in synth.PHYLO_SNPS).encode(), dtype=np.uint8)]
    pick = rng.randint(0, len(pos), n)
    c = pos[pick] - 1                                           # the SNP base, 0-based
    lead = rng.randint(24, 76, n)
    start = c - synth.FLANK - lead
    jj = np.arange(L, dtype=np.int64)
    codes = _CODE[g[start[:, None] + jj[None, :]]]
    at = lead + synth.FLANK                                     # the SNP base inside the read
    side = np.where(rng.randint(0, 2, n) == 0, -1, 1)
    first_off = rng.randint(3, 20, n)
    rows = np.arange(n)
    # (a random genome has the template's allele at one SNP in four: the read gets the next letter there)
    codes[rows, at] = np.where(codes[rows, at] == allele[pick], (allele[pick] + 1) % 4, codes[rows, at])
    for k in range(mismatches - 1):
        col = at + side * (first_off + k)
        codes[rows, col] = (codes[rows, col] + rng.randint(1, 4, n)) % 4
    minus = rng.randint(0, 2, n).astype(bool)
    codes = np.where(minus[:, None], 3 - codes[:, ::-1], codes)
    return records_of(_LETTERS[codes], first)


BP_SHARDS = 64                              # shares the tiles of a launch are dealt into (kernels_bp.hip)


def draw_order(ntiles, wg=0):
    """The order in which ONE scan workgroup (KVQ_GRID=1: nobody to race with) takes the tiles of a launch -- NOT the order of the
    text.  kernels_bp.hip: share sh holds the tiles [sh * ntiles / 64, (sh + 1) * ntiles / 64) and a counter; the workgroup starts in
    share blockIdx.x % 64, draws two tiles ahead (bp_draw_wave twice), then one more during every tile from the share it is in
    (atomicAdd on its counter) and, when that has run out, from the first share with tiles left in ITS order sh + m i mod 64,
    i = 0 .. 63, m = ((blockIdx.x >> 6) * 2 + 37) | 1 (bp_draw_wave)."""
    begin = lambda sh: sh * ntiles // BP_SHARDS
    ctr = [begin(sh) for sh in range(BP_SHARDS)]
    m = ((wg >> 6) * 2 + 37) | 1
    at = [wg % BP_SHARDS]

    def draw_wave():
        for i in range(BP_SHARDS):
            mine = (at[0] + m * i) % BP_SHARDS
            if ctr[mine] < begin(mine + 1):
                ctr[mine] += 1; at[0] = mine
                return ctr[mine] - 1
        return ntiles
    order = []
    g = draw_wave()
    nxt = draw_wave() if g < ntiles else ntiles
    no_more = nxt >= ntiles
    while g < ntiles:
        order.append(g)
        d = ntiles
        if not no_more:
            d = ctr[at[0]]; ctr[at[0]] += 1                     # (drawn while the tile is worked on)
            if d >= begin(at[0] + 1):
                d = draw_wave(); no_more = d >= ntiles
        g, nxt = nxt, d
    return order


def tile_spans(text):
    """[(first byte, first byte behind)] of every tile of a text scanned as one batch, in the order of their numbers (= of the text):
    kvq_seeded_launch counts the tiles of a chunk [a, b) from a & ~15"""
    import kernel_matrix as KM
    from kvarq_amd import scan
    tile, per = KM.tiles_of(text)
    co = [int(x) for x in scan.chunk_offsets(text)]
    out = []
    for (a, b), n in zip(zip(co[:-1], co[1:]), per):
        out += [(max(a, (a & ~15) + k * tile), min(b, (a & ~15) + (k + 1) * tile)) for k in range(n)]
    return out


SILENT_RECORDS = 3400                                           # 28 tiles
SILENT_HEAD_TILES, SILENT_STRETCH_TILES = 6, 16                 # in the order one workgroup draws them: true hits, near-misses; the rest true hits
HEAD, STRETCH, TAIL, NEUTRAL = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def silent_text():
    """-> (text, the class of every record, the stretch's records alone as a text of their own, the draw order of the text's tiles)

    The tiles are given their class by their place in draw_order(): the first SILENT_HEAD_TILES the workgroup takes hold true hits
    (one or two mismatches), the next SILENT_STRETCH_TILES near-misses (maxerrors + 1), the rest true hits again -- in the text
    the three are interleaved.  A record that does not lie wholly inside one tile's bytes is NEUTRAL: random bases, no hit, so
    that it does not matter which of the two tiles makes what of it."""
    rng = np.random.RandomState(70)
    n = SILENT_RECORDS
    neutral = records_of(_LETTERS[rng.randint(0, 4, (n, L))])
    spans = tile_spans(neutral.reshape(-1))
    order = draw_order(len(spans))
    assert len(order) == len(spans) > SILENT_HEAD_TILES + SILENT_STRETCH_TILES + 2
    rank = dict((g, k) for k, g in enumerate(order))
    cls = np.full(n, NEUTRAL, dtype=np.int64)
    g = 0
    for r in range(n):
        while spans[g][1] <= r * RB:
            g += 1
        if spans[g][0] <= r * RB and (r + 1) * RB <= spans[g][1]:
            cls[r] = HEAD if rank[g] < SILENT_HEAD_TILES else STRETCH if rank[g] < SILENT_HEAD_TILES + SILENT_STRETCH_TILES else TAIL
    out = neutral.copy()
    for c, seeds in ((HEAD, (71, 72)), (TAIL, (74, 75))):
        at = np.nonzero(cls == c)[0]
        reads = np.concatenate([snp_reads(len(at) // 2, seeds[0], 1), snp_reads(len(at) - len(at) // 2, seeds[1], 2)])
        out[at] = reads[rng.permutation(len(at))]
    at = np.nonzero(cls == STRETCH)[0]
    stretch = snp_reads(len(at), 73, 3)
    out[at] = stretch
    out[:, :21] = neutral[:, :21]                               # (the names count the records of the text)
    text = out.reshape(-1)
    assert tile_spans(text) == spans, 'the chunk cuts moved with the bases'
    alone = stretch.reshape(-1).copy()
    text.setflags(write=False); alone.setflags(write=False); cls.setflags(write=False)
    return text, cls, alone, tuple(order)


def silent_rounds(alone_slots, block=SV_BLOCK_BESIDE):
    """Whole rounds of ONE workgroup of `block` threads (KVQ_SV_GRID=1) that emit nothing, at the least, when ONE scan workgroup
    (KVQ_GRID=1) takes the stretch's tiles one behind the other (draw_order: silent_text lays them out so) and the stretch's
    records alone gave `alone_slots` slots.

    While the workgroup works on the stretch's tiles it meets near-misses and neutral records only.  The chunks its waves take
    during that time have consecutive numbers (one workgroup: the list's counter moves in time), and there are at least
    alone_slots / 16 - 16 of them: alone, the same items round up to a chunk per wave more, and here a wave's first items go
    into the chunk it had open (up to 15 each, OPEN_CHUNKS waves).  So the range is alone_slots - 2 * 8 * 16 slots or more;
    the rounds that lie wholly inside it number range // block - 1 at the least.  All of their slots are near-misses but for
    the chunk each of the eight waves still has open when the true hits begin again: such a chunk may lie anywhere in the
    range (a wave that found little took it early), so up to eight rounds are given up for them."""
    rng = alone_slots - 2 * OPEN_CHUNKS * SV_CHUNK
    return max(0, rng // block - 1) - OPEN_CHUNKS


# ---------------------------------------------------------------------------------------------------------------
# the round loop of kvq_verify_survivors
# ---------------------------------------------------------------------------------------------------------------

def round_walk(n, grid, block, wrong=None):
    """{workgroup: [the slots of its round 0, of its round 1, ...]} for a list of n slots: kernels_bp.hip,
    ``for (base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x)``, thread t looks at slot base + t < n.

    wrong: a misstatement -- 'step' (base += blockDim.x alone), 'first' (base starts at blockIdx.x), 'loop<=' (base <= n),
    'slot<=' (base + t <= n)"""
    out = {}
    for wg in range(grid):
        rounds = []
        base = wg if wrong == 'first' else wg * block
        while base <= n if wrong == 'loop<=' else base < n:
            rounds.append([base + t for t in range(block) if (base + t <= n if wrong == 'slot<=' else base + t < n)])
            base += block if wrong == 'step' else grid * block
        out[wg] = rounds
    return out


WRONG_WALKS = ('step', 'first', 'loop<=', 'slot<=')


def rounds_per_workgroup(n, grid, block):
    """(most, fewest) rounds a workgroup walks"""
    k = [len(r) for r in round_walk(n, grid, block).values()]
    return max(k), min(k)


def walk_is_exact(walk, n, grid, block):
    """every slot once, and no round more than the list needs"""
    seen = sorted(s for rounds in walk.values() for r in rounds for s in r)
    per = grid * block
    return seen == list(range(n)) and all(len(walk[wg]) == max(0, -(-(n - wg * block) // per)) for wg in range(grid))
