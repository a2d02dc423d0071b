"""
The inputs of tests/results_matrix.py against the oracle alone (no GPU): each text has the shape its seam of the finish
tail needs -- tests/test_gpu_results.py then runs them through the library -- and the reference itself stays within
every stated condition.
"""
import collections

import numpy as np

import results_matrix as M


def counts(ref):
    return [c for _, c in M.hits_per_read(ref.file_pos)]


def record_lengths(text):
    return [e - a for a, _, _, e in M.split_records(text)]


def test_the_ladder_yields_every_occupancy_from_1_to_64_and_the_hit_lengths_at_the_folds_seams():
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    per = collections.Counter(counts(ref))
    assert sorted(per) == list(range(1, 65)) and set(per.values()) == {M.LADDER_ROUNDS}
    # every read has a hit; the records stay within a factor of two of each other
    assert len(M.split_records(text)) == len(counts(ref)) == 64 * M.LADDER_ROUNDS
    ln = record_lengths(text)
    assert max(ln) <= 2 * min(ln)
    assert 100000 < len(text) < 2 << 20
    # hit lengths around the fold's 16-byte step and its 4-byte words, and one long hit
    lengths = set(ref.length.tolist())
    assert {1, 2, 3, 15, 16, 17, 31, 32, 33} <= lengths and max(lengths) >= 40
    assert ref.length.tolist() == [len(h) for h in ref.hitseqs]
    # class A (the read's tail on the sequence's head: seq_pos < 0, cut at the read's end), class B (the read's head on the
    # sequence's tail: seq_pos > 0, cut at the sequence's end), class C with seq_pos < 0
    seql = np.array([len(s) for s in seqs])[ref.seq_nr]
    a = (ref.seq_pos < 0) & (ref.length < seql) & (-ref.seq_pos + ref.length == ref.readlength)
    b = (ref.seq_pos > 0) & (ref.seq_pos + ref.length == seql)
    c = (ref.seq_pos < 0) & (ref.length == seql)
    assert a.sum() >= M.LADDER_ROUNDS and b.sum() >= M.LADDER_ROUNDS and c.sum() > 1000
    # no bucket of the ordering holds two reads (the bucket is narrower than a record): occupancy == hits per read
    shift, nb, bc = M.plan_geometry(0, len(text), ref.n)
    assert (1 << shift) <= min(ln)
    per_bucket, per_share = M.occupancy(ref.file_pos, 0, shift, bc, nb)
    assert sorted(per_bucket[per_bucket > 0].tolist()) == sorted(counts(ref))
    assert int(per_share.sum()) == ref.n


def test_the_read_of_65_hits_makes_one_crowded_bucket_first_in_the_middle_and_last():
    base = M.ref_of('ladder')
    firsts = {}
    for where in ('first', 'middle', 'last'):
        text, _ = M.ladder65(where)
        ref = M.ref_of('ladder65', where)
        per = M.hits_per_read(ref.file_pos)
        assert ref.n == base.n + 65 and sorted(c for _, c in per)[-2:] == [64, 65]
        firsts[where] = [i for i, (_, c) in enumerate(per) if c == 65]
        shift, nb, bc = M.plan_geometry(0, len(text), ref.n)
        per_bucket, _ = M.occupancy(ref.file_pos, 0, shift, bc, nb)
        assert int(per_bucket.max()) == 65 and int((per_bucket > M.BUCKET_MAX).sum()) == 1
        # (a text's first hit lies behind its record's name line: with buckets of a few bytes that is not bucket 0)
        if where == 'first':
            assert int(np.nonzero(per_bucket)[0][0]) == int(np.argmax(per_bucket)) < 8
        if where == 'last':
            assert int(np.nonzero(per_bucket)[0][-1]) == int(np.argmax(per_bucket)) > nb - 512
    assert firsts == {'first': [0], 'middle': [32 * M.LADDER_ROUNDS], 'last': [64 * M.LADDER_ROUNDS]}


def test_the_ties_differ_only_in_class_or_ordinal_in_both_regimes():
    for regime, lo, hi in (('wave', 9, 64), ('network', 2, 8)):
        text, seqs = M.ties(regime)
        ref = M.ref_of('ties', regime)
        per = counts(ref)
        assert len(per) == len(M.split_records(text)) >= 100 and lo <= min(per) and max(per) <= hi
        # per (file_pos, seq_nr): several hits, of more than one class
        groups = collections.defaultdict(list)
        for i in range(ref.n):
            groups[(int(ref.file_pos[i]), int(ref.seq_nr[i]))].append((int(ref.seq_pos[i]), int(ref.length[i])))
        assert min(len(g) for g in groups.values()) >= 2
        assert int(ref.readlength.min()) > max(len(s) for s in seqs)      # (every sequence lies whole inside a read: class C has its length)
        mixed = 0
        for (_, s), g in groups.items():
            assert len(set(g)) == len(g)
            full = len(seqs[s])
            classes = {'C' if ln == full else 'A' if sp < 0 else 'B' for sp, ln in g}
            mixed += len(classes) > 1
        assert mixed >= len(groups) // 2
        shift, nb, bc = M.plan_geometry(0, len(text), ref.n)
        per_bucket, _ = M.occupancy(ref.file_pos, 0, shift, bc, nb)
        assert sorted(per_bucket[per_bucket > 0].tolist()) == sorted(per)


def test_the_dense_corner_crowds_a_sixteenth_of_the_reads_into_a_few_shares():
    text, _ = M.dense_corner()
    ref = M.ref_of('dense_corner')
    ln = record_lengths(text)
    assert len(ln) == M.DENSE_READS and 90 <= min(ln) == max(ln) <= 110 and len(text) < 2 << 20
    per = M.hits_per_read(ref.file_pos)
    assert [c for _, c in per] == [32] * (M.DENSE_READS // 16)
    recs = M.split_records(text)
    assert [fp for fp, _ in per] == [recs[i][1] for i in range(*M.DENSE_HOT)]          # one contiguous sixteenth
    shift, nb, bc = M.plan_geometry(0, len(text), ref.n)
    per_bucket, per_share = M.occupancy(ref.file_pos, 0, shift, bc, nb)
    assert int(per_bucket.max()) == 32
    assert nb % bc != 0
    assert int(per_share.max()) > 2 * M.GATHER_CHUNK                                       # several chunks of the gather ...
    assert any(c > 2 * M.GATHER_CHUNK and c % M.GATHER_CHUNK for c in per_share.tolist())  # ... with a ragged last one
    assert int((per_share == 0).sum()) > M.ORDER_BLOCKS * 7 // 8                           # most shares are empty
    assert (M.ORDER_BLOCKS - 1) * bc >= nb                                                 # the last share lies behind the last bucket


def test_the_tiny_texts_have_0_1_and_2_hits_and_one_in_the_last_bucket():
    want = {'zero': [], 'one': [1], 'two_in_one': [2], 'first_and_last': [1, 1]}
    for which in M.TINY:
        text, _ = M.tiny(which)
        ref = M.ref_of('tiny', which)
        assert counts(ref) == want[which] and ref.records_parsed == 500
        assert ref.offsets.tolist()[0] == 0 and len(ref.offsets) == ref.n + 1
    text, _ = M.tiny('first_and_last')
    ref = M.ref_of('tiny', 'first_and_last')
    recs = M.split_records(text)
    assert ref.file_pos.tolist() == [recs[0][1], recs[-1][1]]
    shift, nb, bc = M.plan_geometry(0, len(text), 2)
    per_bucket, _ = M.occupancy(ref.file_pos, 0, shift, bc, nb)
    assert per_bucket[0] == 1 and per_bucket[nb - 1] == 1


def test_the_offset_batches_are_the_ladder_cut_at_a_record_with_a_gap_far_from_zero():
    text, _ = M.ladder()
    (p0, b0), (p1, b1) = M.offset_batches()[0]
    assert p0 + p1 == text and p0.endswith(b'\n') and p1.startswith(b'@') and len(p0) > 1000 < len(p1)
    assert b0 == (1 << 33) + 12345 and b1 - (b0 + len(p0)) > 1 << 20
    ref, whole = M.offset_reference(), M.ref_of('ladder')
    # the same hits as the whole text's, moved: the oracle's result per piece with the bases added
    moved = np.where(whole.file_pos < len(p0), whole.file_pos + b0, whole.file_pos - len(p0) + b1)
    assert ref.file_pos.tolist() == moved.tolist() and ref.hitseqs == whole.hitseqs
    assert ref.coverage.tolist() == whole.coverage.tolist() and ref.nseqhits.tolist() == whole.nseqhits.tolist()
    assert ref.file_pos.min() > 1 << 33


def test_the_fold_text_counts_every_mutation_class_at_the_named_offsets():
    text, seqs = M.fold()
    ref = M.ref_of('fold')
    assert M.FOLD_CFG['maxerrors'] > 0 and [len(s) for s in seqs] == [64, 65, 127, 128]
    assert ref.n > 500 and ref.n % 64 != 0
    assert len(M.split_records(text)) == len(counts(ref))                   # only reads the oracle confirms
    # all six classes of read bytes (A, C, G, T, N, another letter)
    assert (ref.mutations.reshape(-1, 6).sum(axis=0) > 0).all()
    mm = M.mismatch_offsets(ref)
    assert 1 <= min(len(m) for m in mm) and max(len(m) for m in mm) <= 2
    seen = {o for m in mm for o in m}
    assert {0, 3, 4, 15, 16} <= seen
    assert sum(1 for i, m in enumerate(mm) if m[-1] == int(ref.length[i]) - 1) > 50      # ... and on the hit's last base
    # every sequence: hits that cover its last base (the coverage's end mark), mutations on its first and last base
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    mut = ref.mutations.reshape(-1, 6).sum(axis=1)
    for s in range(len(seqs)):
        assert ref.coverage[off[s + 1] - 1] > 0 and ref.coverage[off[s]] > 0
        assert mut[off[s]] > 0 and mut[off[s + 1] - 1] > 0
        for o in (3, 4, 15, 16):
            assert mut[off[s] + o] > 0
    # one hit ends on the last base of the last sequence of the table
    last = len(seqs) - 1
    ends = np.maximum(ref.seq_pos, 0) + ref.length
    assert ((ref.seq_nr == last) & (ends == len(seqs[last]))).any()
    # classes A (seq_pos < 0, cut at the read's end) and B (they end on the sequence's last base) among them
    seql = np.array([len(s) for s in seqs])[ref.seq_nr]
    assert ((ref.seq_pos < 0) & (ref.length < seql)).any() and ((ref.seq_pos > 0) & (ref.seq_pos + ref.length == seql)).any()


def test_plan_geometry_at_its_corners():
    # no hit, one hit, two: 256 buckets of the narrowest width that covers the span
    assert M.plan_geometry(0, 1, 0) == (0, 2, 1)
    assert M.plan_geometry(0, 255, 1) == (0, 256, 1)
    assert M.plan_geometry(0, 256, 2) == (1, 129, 1)
    assert M.plan_geometry(1 << 33, (1 << 33) + 65536, 2) == (9, 129, 1)
    # four buckets per hit, at most what the arena's capacity gives
    assert M.plan_geometry(0, 1 << 20, 1000) == (9, 2049, 5)
    assert M.plan_geometry(0, 1 << 20, 1000, arena_cap=64) == (13, 129, 1)
