"""
The BAM record decoder's kernels at their seams on an MI355X (kernels_bam.hip): kvq_bam_run_device --
kvq_bam_find, the chain check and kvq_bam_emit as the route calls them -- against the run reference of tests/bam_seams.py
(proven against the host twin in tests/test_bam_seams_host.py), byte for byte and report field by field: every segment
size of a sweep, every kind of text byte on both sides of the writer's 4 KiB window at every alignment of the output,
fake chains that break, overshoot, sit in the cut record or in front of a malformed one, a run cut at every byte with
and without the rest of the stream behind it, every rule through the kernels, and on the route a run boundary at a chosen
byte of a record.  The output lies inside a patterned buffer, and every byte outside the text must keep the pattern.
"""
import ctypes as C

import pytest

import bam_seams as S
import bam_writer as W
import cases
from kvarq_amd import _lib, bam, engine, synth
from test_bam_host import corpus
from test_bam_seams_host import check_broken_cut, counts
from test_gpu_bam import _three_way

pytestmark = pytest.mark.gpu

PAD, PATTERN = 64, 0xA5


class Dev(object):
    """a stream in device memory, as it is and with 0xFF behind the cut, and a patterned output buffer around the text"""

    def __init__(self, in_cap=1 << 17, text_cap=1 << 18):
        L = self.L = _lib.lib()
        self.in_cap, self.cap = in_cap, PAD + 16 + text_cap + PAD
        self.d = [L.kvq_device_alloc(in_cap), L.kvq_device_alloc(in_cap)]
        self.d_out = L.kvq_device_alloc(self.cap)
        assert self.d[0] and self.d[1] and self.d_out
        self.host = C.create_string_buffer(self.cap)
        self.data, self.calls = None, 0

    def load(self, data):
        if data is self.data:
            return self
        assert len(data) <= self.in_cap
        for d in self.d:
            assert self.L.kvq_memcpy_h2d(d, data, len(data)) == 0
        self.data, self.ff_from = data, len(data)
        return self

    def _ff(self, cut):
        """the second copy holds data[:cut] and 0xFF behind it"""
        if cut > self.ff_from:
            assert self.L.kvq_memcpy_h2d(self.d[1], self.data, len(self.data)) == 0
            self.ff_from = len(self.data)
        if cut < self.ff_from:
            assert self.L.kvq_memset_d(C.c_void_p(self.d[1] + cut), 0xFF, self.ff_from - cut) == 0
            self.ff_from = cut

    def run(self, data, cut, first, n_ref, base=0, sb=None, out_off=PAD, ff=False):
        """kvq_bam_run_device on the buffer data[base:cut] of the stream: (return value, end, text, report), offsets
        relative to the stream; the bytes of the output buffer outside the text must hold the pattern afterwards"""
        L = self.L
        self.calls += 1
        self.load(data)
        if ff:
            self._ff(cut)
        assert L.kvq_memset_d(self.d_out, PATTERN, self.cap) == 0
        p = C.c_void_p(self.d[1 if ff else 0] + base)
        try:
            t, end, rep = bam.run_device(p, cut - base, len(data) - base, n_ref, first - base, self.d_out, out_off, self.cap, sb)
        except bam.BamError as e:
            t, end, rep = -1, e.end, e.report
        assert L.kvq_memcpy_d2h(self.host, self.d_out, self.cap) == 0
        got, w = self.host.raw, max(t, 0)
        assert got[:out_off] == bytes([PATTERN]) * out_off, 'a store in front of the text'
        assert got[out_off + w:] == bytes([PATTERN]) * (self.cap - out_off - w), 'a store behind the text'
        assert rep['runs'] == 1 and (t < 0 or (rep['bam_bytes'], rep['text_bytes']) == (cut - base, t))
        return t, end + base, got[out_off:out_off + w], rep

    def free(self):
        for d in self.d + [self.d_out]:
            self.L.kvq_device_free(d)


@pytest.fixture(scope='module')
def dev():
    d = Dev()
    yield d
    print('kvq_bam_run_device: %d calls' % d.calls)
    d.free()


def nseg(n, first, sb):
    return (n - first + sb - 1) // sb if n > first else 0


def same(got, ref, where):
    t, end, text, rep = got
    assert (t, end) == (len(ref.text), ref.end), where
    assert text == ref.text, where
    assert counts(rep) == (ref.seen, ref.written, ref.skipped, ref.noqual), where


def test_segment_sweep(dev):
    data = S.sweep_stream()
    n_ref, first = W.first_record(data)
    ref = S.run_ref(data, first, len(data))
    assert ref.text == W.to_fastq(data) and ref.end == len(data)
    for sb in S.SWEEP_SIZES:
        got = dev.run(data, len(data), first, n_ref, sb=sb)
        same(got, ref, sb)
        assert got[3]['segments'] == nseg(len(data), first, sb) and got[3]['check_passes'] <= got[3]['segments'] + 1, sb


def test_window_sweep(dev):
    by_d = {}
    for d, mis in S.window_cases():
        by_d.setdefault(d, []).append(mis)
    for d, miss in sorted(by_d.items()):
        data = S.window_stream(d)
        n_ref, first = W.first_record(data)
        ref = S.run_ref(data, first, len(data))
        for mis in miss:
            got = dev.run(data, len(data), first, n_ref, sb=len(data) + 1, out_off=PAD + mis)
            same(got, ref, (d, mis))
            assert got[3]['segments'] == 1


def test_alignment_and_segment_edges(dev):
    for data in (S.tiny_stream(), corpus()['mixed']):
        n_ref, first = W.first_record(data)
        ref = S.run_ref(data, first, len(data))
        assert ref.text == W.to_fastq(data)
        for sb in (40, 100, 1024, None):
            for off in range(16):
                same(dev.run(data, len(data), first, n_ref, sb=sb, out_off=off), ref, (len(data), sb, off))


def test_baits(dev):
    for name, b in sorted(S.baits().items()):
        n_ref, first = W.first_record(b.data)
        cut = len(b.data) if b.cut is None else b.cut
        for sb in b.sizes:
            if b.at is None:
                ref = S.run_ref(b.data, first, cut)
                got = dev.run(b.data, cut, first, n_ref, sb=sb)
                same(got, ref, (name, sb))                  # (the cut record a bait: the text from out's first byte on)
                same(dev.run(b.data, cut, first, n_ref, sb=sb, ff=True), ref, (name, sb, 'ff'))
                rep = got[3]
            else:
                t, end, _, rep = dev.run(b.data, cut, first, n_ref, sb=sb)
                assert t == -1 and end == b.at and _lib.last_error() == (_lib.ERR_IO, 'malformed BAM record : offset=%d' % b.at)
            assert rep['segments'] == nseg(cut, first, sb)
            assert rep['refuted'] > 0 and rep['check_passes'] <= rep['segments'] + 1, (name, sb)
            print('bait %-16s segment size %4d: segments %d refuted %d check_passes %d'
                  % (name, sb, rep['segments'], rep['refuted'], rep['check_passes']))


def test_run_cut_at_every_byte(dev):
    data, cuts = S.cut_stream()
    n_ref, first = W.first_record(data)
    whole = W.to_fastq(data)
    for sb in (64, 1024, None):
        for cut in reversed(cuts):
            ref = S.run_ref(data, first, cut)
            got = dev.run(data, cut, first, n_ref, sb=sb)
            same(got, ref, (sb, cut))
            assert got[3]['segments'] == nseg(cut, first, sb or 65536)
            blind = dev.run(data, cut, first, n_ref, sb=sb, ff=True)
            same(blind, ref, (sb, cut, 'ff'))
            assert {k: v for k, v in blind[3].items() if not k.startswith('ms_')} == {k: v for k, v in got[3].items() if not k.startswith('ms_')}
            if sb == 64:
                # the replay: the rest as run 2, from the record run 1 ended inside
                t2, end2, text2, _ = dev.run(data, len(data), got[1], n_ref, base=got[1], sb=sb)
                assert got[2] + text2 == whole and end2 == len(data), cut


@pytest.mark.parametrize('field', S.RULES)
def test_rules_through_the_kernels(dev, field):
    for place, sb in S.PLACES.items():
        b = S.rule_stream(field, place)
        n_ref, first = W.first_record(b.data)

        def run(data, cut, first, n_ref, base=0):
            return dev.run(data, cut, first, n_ref, base=base, sb=sb)
        got = [check_broken_cut(run, b, first, n_ref, cut) for cut in [len(b.data)] + b.cuts]
        assert got[0] == 'fail' and got[1] == 'ok'


# ---- on the route: a run boundary at a chosen byte -------------------------------------------------------------------

@pytest.fixture(scope='module')
def route_text(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('bam_seams') / 'body_virtual.fastq')
    with open(p, 'wb') as f:
        f.write(S.route_body()[2])
    return p


@pytest.mark.parametrize('phase', S.PHASES)
def test_route_run_boundary(tmp_path, monkeypatch, route_text, phase):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    hdr, records, probe, off = S.route_stream(phase)
    data = hdr + b''.join(records)
    cuts = [65280 * i for i in range(1, len(data) // 65280 + 1)]
    sizes = [b - a for a, b in zip([0] + cuts, cuts + [len(data)])]
    # run 1 is the first 32 blocks: a 33rd would pass 2 MiB
    assert sum(sizes[:32]) == S.RUN1 == probe + off <= 2097152 < S.RUN1 + sizes[32] and sizes[32] > 8192
    p = str(tmp_path / (phase + '.bam'))
    assert W.write(p, hdr, records, cuts=cuts, level=1) == data
    seqs = synth.both_strands(synth.table(synth.genome())) + [S.MARKER]
    got = _three_way([p], [route_text], seqs, dict(cases.PRODUCT, nthreads=4))
    rep = engine.last_bam_report()
    assert rep['runs'] == 2 and rep['records_seen'] == len(records) and rep['records_skipped'] == 1
    assert sum(1 for h in got['hits'] if h.seq_nr == len(seqs) - 1) == 3
