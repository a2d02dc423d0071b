#!/usr/bin/env python3
"""End-to-end rate of engine.findseqs on BAM input against the BGZF device route
(section 9) on the same reads.  The bench workload's seeded reads (--reads x 150 bp) become an
unaligned BAM (one record per read: name, 4-bit bases, Phred qualities, flag 0x4) and a BGZF
.fastq.gz of its virtual FastQ text, both in bgzip's 65 280-byte blocks at level 6, so that the two
calls must return the same results (checked).  The two routes are timed alternately, --reps times
each after one warm-up, in this one process; the BAM route's report gives its phase split.

--profile: one call of each route, for a run under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from bgzf_rate import write_bgzf  # noqa: E402
from kvarq_amd import _lib, engine, scan, synth  # noqa: E402

L = 150
HEAD = b'BAM\x01' + (0).to_bytes(4, 'little') + (0).to_bytes(4, 'little')       # no header text, no references


def bam_and_text(data, n):
    """(inflated BAM stream, virtual FastQ text) of n synthetic records ('@SYN.<9 digits> 1:N:0', bases, '+', qualities)"""
    rb = synth.record_bytes(L)
    r = data.reshape(n, rb)
    name, bases, quals = r[:, 1:14], r[:, 21:21 + L], r[:, 24 + L:24 + 2 * L]
    lut = np.zeros(256, np.uint8)
    for c, v in zip(b'=ACMGRSVTWYHKDBN', range(16)):
        lut[c] = v
    codes = lut[bases]
    packed = (codes[:, 0::2] << 4) | codes[:, 1::2]
    fixed = np.frombuffer(np.array([(32 + 14 + L // 2 + L, -1, -1, 14, 255, 4680, 0, 4, L, -1, -1, 0)],
                                   dtype=[('bs', '<i4'), ('ref', '<i4'), ('pos', '<i4'), ('lrn', 'u1'), ('mapq', 'u1'),
                                          ('bin', '<u2'), ('ncig', '<u2'), ('flag', '<u2'), ('lseq', '<i4'), ('nref', '<i4'),
                                          ('npos', '<i4'), ('tlen', '<i4')]).tobytes(), np.uint8)
    rec = np.empty((n, 36 + 14 + L // 2 + L), np.uint8)
    rec[:, :36] = fixed
    rec[:, 36:49] = name
    rec[:, 49] = 0
    rec[:, 50:50 + L // 2] = packed
    rec[:, 50 + L // 2:] = quals - 33
    text = np.empty((n, 1 + 13 + 1 + L + 3 + L + 1), np.uint8)
    text[:, 0] = ord('@'); text[:, 1:14] = name; text[:, 14] = 10
    text[:, 15:15 + L] = bases; text[:, 15 + L:18 + L] = np.frombuffer(b'\n+\n', np.uint8)
    text[:, 18 + L:18 + 2 * L] = quals; text[:, 18 + 2 * L] = 10
    return np.concatenate([np.frombuffer(HEAD, np.uint8), rec.reshape(-1)]), text.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--level', type=int, default=6)
    ap.add_argument('--dir', default='/tmp')
    ap.add_argument('--profile', action='store_true')
    a = ap.parse_args()
    procs = min(16, len(os.sched_getaffinity(0)))
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.', nthreads=16)
    tag = '%dM_l%d' % (a.reads // 1_000_000, a.level)
    bam_path = os.path.join(a.dir, 'kvq_bam_rate_%s.bam' % tag)
    fq_path = os.path.join(a.dir, 'kvq_bam_rate_%s.fastq.gz' % tag)
    if not (os.path.exists(bam_path) and os.path.exists(fq_path)):
        dg = scan.DeviceBuffer(g.nbytes); dg.upload(g)
        dd = scan.DeviceBuffer(a.reads * synth.record_bytes(L))
        _lib.lib().kvq_synth_reads_device(dd.ptr, 0, a.reads, L, synth.SEED, dg.ptr, g.nbytes)
        data = dd.download()
        dd.free(); dg.free()
        t0 = time.perf_counter()
        stream, text = bam_and_text(data, a.reads)
        del data
        print('built %.2f GB of BAM records and %.2f GB of text in %.1f s' % (stream.nbytes / 1e9, text.nbytes / 1e9, time.perf_counter() - t0), flush=True)
        for arr, path in ((stream, bam_path), (text, fq_path)):
            raw = path + '.raw'
            arr.tofile(raw)
            t0 = time.perf_counter()
            write_bgzf(path, raw, arr.nbytes, a.level, procs)
            os.remove(raw)
            print('wrote %s (%.2f GB) in %.1f s' % (path, os.path.getsize(path) / 1e9, time.perf_counter() - t0), flush=True)
        del stream, text
    routes = (('bam', bam_path, 'host', 'device_bam'), ('device', fq_path, 'device', 'device'))
    if a.profile:
        engine.config(**cfg)
        for name, path, inflate, want in routes:
            t0 = time.perf_counter()
            r = engine.findseqs(path, seqs, inflate=inflate)
            assert engine.last_inflate() == want
            print('profile %s: %.3f s  hits=%d' % (name, time.perf_counter() - t0, len(r['hits'])), flush=True)
        return
    times = {r[0]: [] for r in routes}
    reports = []
    ref = None
    for rep in range(a.reps + 1):                                      # rep 0: warm-up (page cache, buffers, kept scan)
        for name, path, inflate, want in routes:
            engine.config(**cfg)
            t0 = time.perf_counter()
            r = engine.findseqs(path, seqs, inflate=inflate)
            dt = time.perf_counter() - t0
            assert engine.last_inflate() == want, (name, engine.last_inflate())
            key = (r['hits'], r['hitseqs'], r['stats']['parsed'], r['stats']['records_parsed'], r['stats']['readlengths'],
                   r['stats']['nseqhits'], r['stats']['nseqbasehits'])
            ref = ref or key
            assert key == ref, name
            if rep:
                times[name].append(dt)
                if name == 'bam':
                    reports.append(engine.last_bam_report())
    text = ref[2]
    for name, path, _, _ in routes:
        ts = times[name]
        med = sorted(ts)[len(ts) // 2]
        row = dict(route=name, reads=a.reads, text_bytes=text, file_bytes=os.path.getsize(path), seconds=ts, median_s=med,
                   reads_per_s=a.reads / med, text_GB_per_s=text / med / 1e9, hits=len(ref[0]))
        print('%-7s median %.3f s (best %.3f)  %.1f M reads/s  %.2f GB/s of text  hits=%d  results equal'
              % (name, med, min(ts), a.reads / med / 1e6, text / med / 1e9, len(ref[0])), flush=True)
        print(json.dumps(row), flush=True)
    mid = sorted(reports, key=lambda r: r['ms_inflate'] + r['ms_find'] + r['ms_emit'])[len(reports) // 2]
    bam_med = sorted(times['bam'])[len(times['bam']) // 2] * 1e3
    rest = bam_med - mid['ms_inflate'] - mid['ms_find'] - mid['ms_emit']
    print('bam phases (median report): inflate %.1f ms  find+check %.1f ms  emit %.1f ms  scan, cuts and the rest %.1f ms  '
          '(runs %d, segments %d, refuted %d, passes %d, records %d, bam %.2f GB -> text %.2f GB)'
          % (mid['ms_inflate'], mid['ms_find'], mid['ms_emit'], rest, mid['runs'], mid['segments'], mid['refuted'],
             mid['check_passes'], mid['records_written'], mid['bam_bytes'] / 1e9, mid['text_bytes'] / 1e9), flush=True)
    print(json.dumps(dict(bam_report=mid)), flush=True)


if __name__ == '__main__':
    main()
