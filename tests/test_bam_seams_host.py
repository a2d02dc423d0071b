"""
The BAM seam corpus on the CPU (tests/bam_seams.py).  Two things are settled here before the corpus
judges the GPU kernels in tests/test_gpu_bam_seams.py: every stream meets the conditions it was built for (asserted with the
layout model, not hoped for), and the run reference ``run_ref`` agrees with kvq_bam_run_host -- the host twin over the
shared kvq_bam_check -- at every cut of a run, on well-formed and malformed streams, and over replays in several runs.
"""
import ctypes as C
import random

import pytest

import bam_seams as S
import bam_writer as W
from kvarq_amd import _lib, bam


def host_run(data, n, first, n_ref, limit=None, base=0):
    """kvq_bam_run_host on the buffer data[base:n] of a stream that ends at limit: (return value, end, text, report), the
    offsets relative to the stream"""
    L = _lib.lib()
    buf = bytes(data[base:n])                   # nothing behind n is there to be read
    limit = len(data) if limit is None else limit
    end = C.c_int64(-7)
    out = C.create_string_buffer(max(1, 2 * len(buf) + 64))
    t = L.kvq_bam_run_host(buf, len(buf), limit - base, n_ref, first - base, out, len(out), C.byref(end))
    return t, end.value + base, out.raw[:max(t, 0)], bam.last_report()


def counts(rep):
    return rep['records_seen'], rep['records_written'], rep['records_skipped'], rep['records_noqual']


def named(offset):
    return (_lib.ERR_IO, 'malformed BAM record : offset=%d' % offset)


# ---- the conditions ----------------------------------------------------------------------------------------------

def test_segment_sweep_stream_meets_its_conditions():
    data = S.sweep_stream()
    recs = S.walk_cached(data)
    assert 45 <= len(recs) <= 60 and 5000 < len(data) < 16000
    assert b''.join(r.text for r in recs) == W.to_fastq(data)
    met = S.sweep_conditions(data, range(38, 166))
    for name in ('start_at_0', 'start_1_before_end', 'start_2_before_end', 'start_3_before_end', 'fixed_straddles', 'passed_over'):
        assert met[name], name
    print('segment sweep: %d bytes, %d records; sizes that meet each condition: %s'
          % (len(data), len(recs), {k: len(set(v)) for k, v in sorted(met.items())}))
    # the tiny records at a segment size of 40: one record a segment, 9 text bytes each
    tiny = S.tiny_stream()
    assert S.words_from_three_segments(tiny, 40) and all(S.words_from_three_segments(tiny, 40, mis) for mis in range(16))
    assert S.words_from_three_segments(data, 40)


def test_window_sweep_puts_every_kind_of_byte_on_both_sides_of_a_seam():
    cases = S.window_cases()
    got = S.window_coverage(cases)
    for mis in range(16):
        for probe, p in enumerate(S.PROBES):
            kinds = [k for k in S.KINDS]
            for k in kinds:
                for side in ('last', 'first'):
                    assert (mis, probe, k, side) in got, (mis, probe, k, side)
    for d in S.WINDOW_D:
        data = S.window_stream(d)
        texts = [t for _, t in S.window_probe_at(data)]
        assert texts[0] == b'@probe/1\nTCAACGT\n+\n!#JI?5+\n' and texts[1] == b'@probe/1\nTGTAATC\n+\n"""""""\n'
        assert texts[2] == b'@probe/2\nCCGTTGN\n+\nI?5+&"!\n'
        assert len(W.to_fastq(data)) - S.window_probe_at(data)[2][0] > S.WIN + 27
    print('window sweep: %d (d, mis) cases over %d streams' % (len(cases), len(S.WINDOW_D)))


def test_baits_mislead_the_speculation_where_they_were_built_to():
    for name, b in sorted(S.baits().items()):
        n_ref, first = W.first_record(b.data)
        cut = len(b.data) if b.cut is None else b.cut
        for sb in b.sizes:
            refuted, emptied = S.speculation_misled(b.data, first, cut, sb)
            assert refuted, (name, sb)
            print('bait %s at segment size %d: segments misled: to walk again %s, to empty %s' % (name, sb, refuted, emptied))
            if name == 'cut_record':
                # a misled segment inside the cut record: a fake chain with text that the host must empty
                assert any(first + k * sb > S.run_ref(b.data, first, cut).end for k in emptied), sb
    b = S.baits()['cut_record']
    n_ref, first = W.first_record(b.data)
    ref = S.run_ref(b.data, first, b.cut)
    # the cut record is the bait, and whole fake records lie between its start and the cut
    assert ref.end < b.cut and ref.text and len(ref.text) < len(W.to_fastq(b.data))
    fake = [o for o in range(ref.end + 1, b.cut) if S.check(b.data, b.cut, len(b.data), n_ref, o)[0] == S.OK]
    assert len(fake) >= 4
    b = S.baits()['before_malformed']
    with pytest.raises(W.Malformed) as e:
        W.to_fastq(b.data)
    assert e.value.offset == b.at


@pytest.mark.parametrize('field', S.RULES)
def test_rule_streams_put_the_bad_record_where_they_say(field):
    for place, sb in S.PLACES.items():
        b = S.rule_stream(field, place)
        n_ref, first = W.first_record(b.data)
        with pytest.raises(W.Malformed) as e:
            W.to_fastq(b.data)
        assert e.value.offset == b.at, place
        k = (b.at - first) // sb
        if place == 'plain':
            assert k == 0
        elif place == 'later':
            assert k >= 2
        elif place == 'straddle':
            assert first + (k + 1) * sb == b.at + 20
        else:
            assert S.speculation_misled(b.data, first, len(b.data), sb)[0]
        assert b.cuts[0] < b.at < b.cuts[-1] and b.cuts == list(range(b.cuts[0], b.cuts[-1] + 1))


def test_route_streams_put_the_run_boundary_on_each_phase():
    recs, m, body = S.route_body()
    for phase in S.PHASES:
        hdr, records, probe, off = S.route_stream(phase)
        data = hdr + b''.join(records)
        assert W.to_fastq(hdr + records[0]) == b''                      # the filler writes nothing: the text is the body's
        assert data[probe:probe + S._REC] == recs[m] and S.MARKER in W.to_fastq(hdr + recs[m])
        assert probe + off == S.RUN1 and len(data) - 32 * 65280 > 8192 and 33 * 65280 > 2097152 >= 32 * 65280
        assert all(len(r) < (1 << 20) for r in records)


# ---- the reference against the host twin ---------------------------------------------------------------------------

def test_run_host_equals_the_reference_at_every_cut():
    data, cuts = S.cut_stream()
    n_ref, first = W.first_record(data)
    whole = W.to_fastq(data)
    seen_kinds = set()
    for cut in cuts:
        ref = S.run_ref(data, first, cut)
        t, end, text, rep = host_run(data, cut, first, n_ref)
        assert (t, end, text) == (len(ref.text), ref.end, ref.text), cut
        assert counts(rep) == (ref.seen, ref.written, ref.skipped, ref.noqual), cut
        assert rep['bam_bytes'] == cut and rep['text_bytes'] == t
        seen_kinds.add((end == cut, t == 0))
        # the replay: the rest as run 2
        t2, end2, text2, _ = host_run(data, len(data), end, n_ref, base=end)
        assert text + text2 == whole and end2 == len(data), cut
    assert (True, False) in seen_kinds and (False, False) in seen_kinds and (True, True) in seen_kinds
    # bad arguments
    L = _lib.lib()
    assert L.kvq_bam_run_host(data, 100, 99, n_ref, first, None, 0, None) == -2
    assert _lib.last_error() == (_lib.ERR_RUNTIME, 'kvq_bam_run_host: bad arguments')
    assert L.kvq_bam_run_host(data, first - 1, len(data), n_ref, first, None, 0, None) == -2
    assert L.kvq_bam_to_fastq_host(data, -1, n_ref, first, None, 0, None) == -2
    assert _lib.last_error() == (_lib.ERR_RUNTIME, 'kvq_bam_to_fastq_host: bad arguments')


def check_broken_cut(run, b, first, n_ref, cut):
    """one cut of a malformed stream through `run` (host_run's signature), the replay included"""
    must_fail, must_succeed, ok = S.broken_ref(b.data, b.at, b.bad_end, first, cut)
    t, end, text, rep = run(b.data, cut, first, n_ref)
    if t == -1:
        assert not must_succeed and _lib.last_error() == named(b.at) and end == b.at, cut
        return 'fail'
    assert not must_fail and (t, end, text) == (len(ok.text), ok.end, ok.text), cut
    assert counts(rep) == (ok.seen, ok.written, ok.skipped, ok.noqual), cut
    t2, end2, _, _ = run(b.data, len(b.data), end, n_ref, base=end)
    assert t2 == -1 and _lib.last_error() == named(b.at - end) and end2 == b.at, cut      # (run 2 counts from its own front)
    return 'ok'


@pytest.mark.parametrize('field', S.RULES)
def test_run_host_names_the_bad_record_at_every_cut_and_in_the_replay(field):
    for place in S.PLACES:
        b = S.rule_stream(field, place)
        n_ref, first = W.first_record(b.data)
        got = [check_broken_cut(host_run, b, first, n_ref, cut) for cut in b.cuts + [len(b.data)]]
        assert got[0] == 'ok' and got[-1] == 'fail'
        # once the verdict is BAD it stays BAD as more bytes come
        assert got == sorted(got, key=lambda g: g == 'fail')


def test_replay_in_several_runs_carries_a_record_through_more_than_one():
    data, _ = S.cut_stream()
    n_ref, first = W.first_record(data)
    whole = W.to_fastq(data)
    recs = S.walk_cached(data)
    long_ = max(recs, key=lambda r: r.end - r.offset)
    rnd = random.Random(9)
    carried = 0
    for trial in range(40):
        k = rnd.randint(3, 6)
        cuts = sorted(set([rnd.randint(long_.offset + 1, long_.end - 1) for _ in range(2)] +
                          [rnd.randint(first + 1, len(data) - 1) for _ in range(k - 3)])) + [len(data)]
        base, start, texts = 0, first, []
        for cut in cuts:
            ref = S.run_ref(data, start, cut)
            t, end, text, _ = host_run(data, cut, start, n_ref, base=base)
            assert (t, end, text) == (len(ref.text), ref.end, ref.text), (cuts, cut)
            if base == long_.offset and end == base:
                carried += 1
                assert text == b''
            texts.append(text)
            base = start = end
        assert b''.join(texts) == whole and base == len(data)
    assert carried > 0


def test_baits_through_the_host_run():
    for name, b in sorted(S.baits().items()):
        n_ref, first = W.first_record(b.data)
        cut = len(b.data) if b.cut is None else b.cut
        if b.at is None:
            ref = S.run_ref(b.data, first, cut)
            t, end, text, rep = host_run(b.data, cut, first, n_ref)
            assert (t, end, text) == (len(ref.text), ref.end, ref.text), name
        else:
            assert check_broken_cut(host_run, S.Broken(b.data, b.at, b.bad_end, None), first, n_ref, cut) == 'fail'
