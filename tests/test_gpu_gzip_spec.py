"""
GPU checks of plain-gzip inflate by speculative chunk decoding: the kernels
through kvq_inflate_gzip_device against the CPU run of the same algorithm (kvq_inflate_gzip_host) --
candidates, chunk ends, text and report --, and findseqs(..., inflate='device_any') against
inflate='host' and the oracle.  Every route test asserts last_inflate(), so that a call that fell
back to the host reader cannot pass.
"""
import gzip
import random
import threading
import time
import zlib

import numpy as np
import pytest

import cases
import inflate_corpus as IC
from kvarq_amd import engine, gzip_spec as G, scan, synth
from oracle import oracle as O
from test_gzip_spec_host import _planted_stream, host_reader
from test_host_logic import bgzf
import deflate_writer as W

pytestmark = pytest.mark.gpu

PAD = 4096
CANARY = 0x5A


def _device(data, chunk_bytes, cap=None):
    """kvq_inflate_gzip_device on data with the text buffer between canaries -> (text, report, chunks) or GzipError"""
    cap = cap if cap is not None else max(1, 6 * len(data) + 65536)
    d_in, d_out = scan.DeviceBuffer(max(1, len(data))), scan.DeviceBuffer(cap + 2 * PAD)
    try:
        if data:
            d_in.upload(np.frombuffer(data, np.uint8))
        d_out.upload(np.full(cap + 2 * PAD, CANARY, np.uint8))
        got, rep = scan.inflate_gzip_device(d_in.ptr, len(data), chunk_bytes, d_out.ptr + PAD, cap)
        out = d_out.download()
        hi = PAD + min(got, cap) if got <= cap else PAD
        assert (out[:PAD] == CANARY).all() and (out[hi:] == CANARY).all(), 'write outside the text'
        return out[PAD:PAD + got].tobytes() if got <= cap else None, rep, G.last_chunks()
    finally:
        d_in.free()
        d_out.free()


def _same_as_host(data, chunk_bytes, seen=None):
    """the device run equals the host run, every chunk slot of both between canaries.  seen(chunks): a check of the caller's on
    the device run's last_chunks(), made in front of the comparison"""
    G.slot_canaries(256)
    try:
        h_text, h_rep = G.inflate_host(data, chunk_bytes)
        h_chunks = G.last_chunks()
        d_text, d_rep, d_chunks = _device(data, chunk_bytes, cap=len(h_text) + 4096)
    finally:
        assert G.slot_canaries(0) == 0, 'a decode wrote outside its slot'
    if seen:
        seen(d_chunks)

    assert d_text == h_text == host_reader(data)
    counts = lambda r: {k: v for k, v in r.items() if not k.startswith("ms_")}
    assert counts(d_rep) == counts(h_rep)
    for a, b in zip(d_chunks, h_chunks):
        assert list(a) == list(b)
    return d_rep


def test_device_stages_equal_the_host_run():
    t = IC.fastq_text(300000)
    for z in (gzip.compress(t, 1), gzip.compress(t, 9), gzip.compress(t[:100000], 6) + gzip.compress(b'', 6) + gzip.compress(t[100000:], 6)):
        for cb in (1024, 16384):
            rep = _same_as_host(z, cb)
            assert rep['chunks'] > 1 and rep['marker_symbols'] > 0


def test_device_refutes_planted_false_positives_and_overflows_slots():
    z, text = _planted_stream()
    seen = 0
    for cb in (256, 512, 1000):
        seen += _same_as_host(z, cb)['refuted']
    assert seen >= 1
    rep = _same_as_host(gzip.compress(b'ACGT' * 200000, 9), 64)
    assert rep['slot_overflows'] >= 1


def _corrupt(z, z2):
    """z and then z2 with one bit of its first block header flipped, the first flip zlib refuses: an error a member in"""
    for at in range(10, 40):
        for bit in range(8):
            bad = bytearray(z2)
            bad[at] ^= 1 << bit
            try:
                host_reader(z + bytes(bad))
            except zlib.error:
                return z + bytes(bad)
    raise AssertionError('no flip fails')


def test_device_truncated_trailing_and_corrupt():
    z = gzip.compress(IC.fastq_text(80000), 6, mtime=0)
    _same_as_host(z[:-5000], 1024)
    _same_as_host(z + b'x' * 11, 1024)
    bad = _corrupt(z, gzip.compress(IC.fastq_text(30000), 6, mtime=0))
    with pytest.raises(G.GzipError) as eh:
        G.inflate_host(bytes(bad), 1024)
    with pytest.raises(G.GzipError) as ed:
        _device(bytes(bad), 1024)
    assert (ed.value.status, ed.value.fpos, str(ed.value)) == (eh.value.status, eh.value.fpos, str(eh.value))


def test_text_that_does_not_fit_is_not_written():
    z = gzip.compress(IC.fastq_text(50000), 6)
    text, _, _ = _device(z, 1024, cap=1000)
    assert text is None


# ---- findseqs(inflate='device_any') ----

def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


def _run(files, seqs, inflate):
    try:
        r = engine.findseqs(files, seqs, inflate=inflate)
        return ('ok', r['hits'], r['hitseqs'], r['stats']), engine.last_inflate()
    except Exception as e:
        return ('err', type(e).__name__, str(e)), engine.last_inflate()


def _both(files, seqs, route='device_gzip'):
    host, h_route = _run(files, seqs, 'host')
    dev, d_route = _run(files, seqs, 'device_any')
    assert h_route == 'host'
    assert d_route == route
    return host, dev


GOLDEN = ['findseqs', 'paired', 'Amin_H', 'bad_at', 'spoligo_5k', 'quirk', 'empty_file', 'partial_tail', 'long_reads',
          'ragged_two_files', 'multichunk', 'synth20k_mtbc']


@pytest.mark.parametrize('name', GOLDEN)
def test_device_any_equals_the_host_route_on_golden_cases(tmp_path, monkeypatch, name):
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '16')
    case = cases.by_name()[name]
    files = []
    for k, p in enumerate(case.materialize(tmp_path)):
        with open(p, 'rb') as f:
            data = f.read()
        if p.endswith('.gz'):
            data = gzip.decompress(data)
        files.append(_write(tmp_path, '%s_%d.fastq.gz' % (name, k), gzip.compress(data, 6)))
    engine.config(**case.config)
    host, dev = _both(files, case.seq_bytes())
    assert dev == host


def test_device_any_over_several_runs_mixed_with_bgzf_equals_host_and_oracle(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')            # runs of 512 KiB compressed: windows carried across runs
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '32')
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    r1, r2, r3 = (synth.reads(g, a, n, 150).tobytes() for a, n in ((0, 30000), (90000, 20000), (150000, 8000)))
    a = _write(tmp_path, 'r_1.fastq.gz', gzip.compress(r1, 1))
    b = _write(tmp_path, 'r_2.fastq.gz', bgzf(r2))
    c = _write(tmp_path, 'r_3.fastq.gz', gzip.compress(r3[:500000], 9) + gzip.compress(r3[500000:], 6) + b'\0' * 12)
    cfg = dict(cases.PRODUCT, nthreads=8)
    engine.config(**cfg)
    host, dev = _both([a, b, c], seqs)
    assert dev == host and dev[0] == 'ok' and len(dev[1]) > 50
    rep = engine.last_inflate_report()
    assert rep['runs'] > 4 and rep['chunks'] > rep['runs']
    o = O.findseqs([a, b, c], seqs, **cfg)
    assert tuple(dev[1]) == tuple(o['hits'])
    assert dev[3] == o['stats']
    # all BGZF: the block route, as inflate='device'
    host, dev = _both([b, b], seqs, route='device')
    assert dev == host


def test_plain_file_in_the_list_takes_the_host_route(tmp_path):
    t = cases.multichunk()
    a = _write(tmp_path, 'a.fastq.gz', gzip.compress(t))
    p = _write(tmp_path, 'p.fastq', t)
    engine.config(**cases.PRODUCT)
    host, dev = _both([a, p], cases.MULTI_SEQS, route='host')
    assert dev == host


def test_device_any_hit_arena_overflow_rescans(tmp_path):
    read = 'ACG' * 60
    data = cases.rec('x', read, 'I' * len(read)) * 40000
    p = _write(tmp_path, 'acg.fastq.gz', gzip.compress(data, 6))
    engine.config(**dict(cases.DEFAULTS, minreadlength=10))
    host, dev = _both([p], [b'ACG'])
    assert dev[0] == 'ok' and len(dev[1]) == 40000 * 60
    assert dev == host


def test_corrupt_stream_raises_ioerror(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '16')
    t = cases.multichunk()
    p = _write(tmp_path, 'bad.fastq.gz', _corrupt(gzip.compress(t, 6, mtime=0), gzip.compress(t[:200000], 6, mtime=0)))
    engine.config(**cases.PRODUCT)
    host, dev = _both([p], cases.MULTI_SEQS)
    assert host[0] == dev[0] == 'err' and host[1] == dev[1] == 'OSError'
    pre = lambda m: m.rsplit(' fpos=', 1)[0]
    assert pre(dev[2]) == pre(host[2]) and 'status=-3' in dev[2]


def test_stop_ends_a_device_any_call(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    data = cases.multichunk() * 20
    p = _write(tmp_path, 'big.fastq.gz', gzip.compress(data, 1))
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    empty = _write(tmp_path, 'empty.fastq', b'')
    engine.findseqs(empty, cases.MULTI_SEQS)
    out = {}

    def run():
        try:
            out['r'] = engine.findseqs(p, cases.MULTI_SEQS, inflate='device_any')
        except Exception as e:
            out['e'] = e
    th = threading.Thread(target=run)
    th.start()
    t0 = time.time()
    while th.is_alive() and time.time() - t0 < 60:
        if engine.stats()['records_parsed'] > 0:
            break
        time.sleep(0.0005)
    engine.stop()
    th.join()
    assert 'e' not in out, out.get('e')
    assert engine.last_inflate() == 'device_gzip'
    st = out['r']['stats']
    assert 0 < st['records_parsed'] and st['parsed'] < len(data)
    full = engine.findseqs(p, cases.MULTI_SEQS, inflate='device_any')
    assert engine.last_inflate() == 'device_gzip'
    assert tuple(full['hits'][:len(out['r']['hits'])]) == tuple(out['r']['hits'])


def _fastq_records(n, seed):
    """n records of random bases and qualities: about 3.7 bits a byte as literals"""
    rnd = random.Random(seed)
    return b''.join(b'@long_%d\n%s\n+\n%s\n' % (i, bytes(rnd.choices(b'ACGT', k=150)), bytes(rnd.choices(range(33, 75), k=150)))
                    for i in range(n))


def test_run_that_reads_past_its_margin_is_repeated_with_its_window(tmp_path, monkeypatch):
    """a DEFLATE block, and a member header, longer than the 1 MiB margin behind a run: the run is read again with a larger
    margin, and its first chunk -- whose copies reach back into the run before -- still resolves against that run's window"""
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')            # runs of 512 KiB compressed
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '32')
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    t1, t3 = synth.reads(g, 0, 13000, 150).tobytes(), synth.reads(g, 60000, 4000, 150).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = co.compress(t1) + co.flush(zlib.Z_SYNC_FLUSH)         # non-final, byte-aligned, well past the first run
    assert len(head) > 600 << 10
    lit = _fastq_records(9000, 9)
    mid, got = W.build([dict(kind='dynamic', tokens=list(lit), final=False), dict(kind='stored', data=b'', final=False)])
    assert got == lit and len(mid) > 1500 << 10                    # one block of literals, far longer than the margin
    co3 = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = head + mid + co3.compress(t3) + co3.flush()
    block_file = _write(tmp_path, 'long_block.fastq.gz', b'\x1f\x8b\x08\x00\0\0\0\0\x00\xff' + raw + b'\0' * 8)
    # a second member whose FNAME runs 3 MB past the first member's end
    name_file = _write(tmp_path, 'long_name.fastq.gz', gzip.compress(t1, 6, mtime=0) + b'\x1f\x8b\x08\x08\0\0\0\0\x00\xff' +
                       b'n' * (3 << 20) + b'\0' + zlib.compress(t3, 6)[2:-4] + b'\0' * 8)
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    for p, text in ((block_file, t1 + lit + t3), (name_file, t1 + t3)):
        with open(p, 'rb') as f:
            assert host_reader(f.read()) == text
        host, dev = _both([p], seqs)
        assert dev == host and dev[0] == 'ok' and len(dev[1]) > 20
        rep = engine.last_inflate_report()
        assert rep['input_retries'] >= 1 and rep['runs'] >= 3, rep



def test_file_that_hands_over_nothing_on_the_gzip_route(tmp_path, monkeypatch):
    """an empty file, BGZF or plain gzip, between or around files of several batches: it hands no batch to the scan, and the
    batch in flight keeps its text buffer (test_gpu_inflate pins the same for the block route)"""
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '32')
    t1, t2 = cases.multichunk(), cases.ragged(9, 3000, cases.RAGGED_TARGETS)
    pa, pb = _write(tmp_path, 'pa.fastq.gz', gzip.compress(t1, 6)), _write(tmp_path, 'pb.fastq.gz', gzip.compress(t2, 6))
    ba, bb = _write(tmp_path, 'ba.fastq.gz', bgzf(t1)), _write(tmp_path, 'bb.fastq.gz', bgzf(t2, level=1))
    pe, be = _write(tmp_path, 'pe.fastq.gz', gzip.compress(b'')), _write(tmp_path, 'be.fastq.gz', bgzf(b''))
    engine.config(**cases.PRODUCT)
    for files in ([pa, be, bb], [ba, pe, pb], [pe, pa, be]):
        host, dev = _both(files, cases.MULTI_SEQS)             # (asserts the route: a list with a plain gzip file takes the gzip route)
        assert dev[0] == 'ok' and dev == host


def _grow_case(tmp):
    """test_text_buffer_grows_while_a_chunk_is_carried in a process whose text buffers are still as the call makes them"""
    import pathlib
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    reads = synth.reads(g, 0, 10000, 150).tobytes()              # 3.25 MB: more than one run compressed
    one = cases.rec('rep', 'ACGT' * 37 + 'AC', 'I' * 150)
    text = reads + one * (8_000_000 // len(one))
    z = gzip.compress(text, 6)
    assert 512 << 10 < len(gzip.compress(reads, 6)) and len(z) < 1024 << 10 and len(text) < 16_000_000
    p = _write(pathlib.Path(tmp), 'grow.fastq.gz', z)
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    dev, d_route = _run([p], seqs, 'device_any')                  # (first: no call before it has made the buffers larger)
    rep = engine.last_inflate_report()
    host, h_route = _run([p], seqs, 'host')
    assert (h_route, d_route) == ('host', 'device_gzip')
    assert dev[0] == 'ok' and dev == host and len(dev[1]) > 20
    # Two runs: the first ends inside the reads, in the middle of a chunk, and the second holds the rest of the file.  A buffer
    # starts with room for a batch, a chunk and 64 bytes, a quarter more and 256 (DevBuf::ensure): the larger run does not fit
    assert rep['runs'] - rep['input_retries'] == 2
    assert len(text) / 2 > ((2 << 20) + (1 << 20) + 64) * 1.25 + 256
    print('grow case ok')


def test_text_buffer_grows_while_a_chunk_is_carried(tmp_path):
    """the second run of the file inflates to more than the text buffer holds (one record repeated: 8 MB out of 50 KB) while
    the unfinished chunk of the first run sits at the buffer's front: the buffer grows and the chunk moves along.  The buffers
    are kept from call to call and only grow, so the case runs in a fresh process, as its first call."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, KVQ_INFLATE_BATCH_MB='2', KVQ_GZIP_CHUNK_KB='32')      # text buffers of 3 MiB and a bit, runs of 512 KiB compressed
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_gzip_spec as T; T._grow_case(%r)' % (os.path.dirname(here), here, str(tmp_path))
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'grow case ok' in r.stdout, r.stdout + r.stderr
