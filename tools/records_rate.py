#!/usr/bin/env python3
"""What keeping the FastQ records of the hits costs (findseqs(records=True), Scanner(records=True)),
written to profiles/records_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with records off and on, alternately, --reps steps each after two warm-ups: the step (scan to finish,
     wall), the GPU time of the batch's kernels (the gather is the difference), the finish after the kernels (wall),
     hits and record bytes;
 (b) extract_hits on a --gz-reads .fastq.gz (one gzip member) scanned with inflate='device_any': the records kept by
     the scan against the host fallback (Fastq.readrecordat, which inflates the file from its start for every hit),
     timed on its first 50 hits and extrapolated.
"""
import argparse
import gzip
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvarq_amd import _lib, analyse, engine, scan, synth  # noqa: E402
from kvarq_amd.fastq import Fastq  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402

CFG = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')      # kvarq/config.py:2-10


def part_a(args, out):
    L = _lib.lib()
    n, rl = args.reads, 150
    rb = synth.record_bytes(rl)
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g, 'MTBC'))
    d_genome = scan.DeviceBuffer(g.nbytes); d_genome.upload(g)
    d_data = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_data.ptr, 0, n, rl, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    offs = analytic_chunk_offsets(n, rb, rl)
    t = scan.Table(seqs, **CFG)
    sc = {False: scan.Scanner(t), True: scan.Scanner(t, records=True)}
    res = {False: [], True: []}
    info = {}
    for rep in range(args.reps + 2):
        for on in (False, True):
            s = sc[on]
            s.reset()
            L.kvq_device_synchronize()
            t0 = time.perf_counter()
            s.scan_device(d_data.ptr, n * rb, offs)
            L.kvq_device_synchronize()
            t1 = time.perf_counter()
            r = s.finish(hits=False, stats=False)
            t2 = time.perf_counter()
            if rep >= 2:
                res[on].append(((t2 - t0) * 1e3, r['kernel_ms'], (t2 - t1) * 1e3, r['main_kernel_ms']))
            info[on] = (r['n_hits'], L.kvq_scan_record_bytes(s.h))
    med = {on: [statistics.median(x[i] for x in res[on]) for i in range(4)] for on in res}
    out.append('(a) %d reads x %d bp resident, MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
               % (n, rl, args.reps))
    out.append('    records   step ms   batch kernels ms   scan kernel ms   finish after kernels ms   hits   record bytes')
    for on in (False, True):
        out.append('    %-7s   %7.3f   %16.3f   %14.3f   %23.3f   %4d   %d' % ('on' if on else 'off', med[on][0], med[on][1], med[on][3], med[on][2],
                                                                         info[on][0], info[on][1]))
    out.append('    gather (batch kernels on - off): %.3f ms = %.1f %% of the scan kernel; extra finish: %.3f ms; step: %+.1f %%'
               % (med[True][1] - med[False][1], 100 * (med[True][1] - med[False][1]) / med[False][3], med[True][2] - med[False][2],
                  100 * (med[True][0] / med[False][0] - 1)))
    for s in sc.values():
        s.close()
    t.close(); d_data.free(); d_genome.free()


def part_b(args, out):
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g, 'MTBC'))
    text = synth.reads(g, 0, args.gz_reads, 150).tobytes()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'reads.fastq.gz')
        with open(path, 'wb') as f:
            f.write(gzip.compress(text, 1, mtime=0))
        engine.config(**dict(CFG, nthreads=8))
        t0 = time.perf_counter()
        r = engine.findseqs(path, seqs, inflate='device_any', records=True)
        t1 = time.perf_counter()
        assert engine.last_inflate() == 'device_gzip'
        a = analyse.Analyser()
        a.fastq = Fastq(path, variant='Sanger', quiet=True)
        a.hits, a.records = r['hits'], r['records']
        t2 = time.perf_counter()
        a.extract_hits(os.path.join(tmp, 'kept.fastq'))
        t3 = time.perf_counter()
        k = min(50, len(r['hits']))
        a.hits, a.records = r['hits'][:k], None
        t4 = time.perf_counter()
        a.extract_hits(os.path.join(tmp, 'fallback.fastq'))
        t5 = time.perf_counter()
        t6 = time.perf_counter()
        a.fastq.readrecordat(r['hits'][-1])                          # (the last hit: the file inflated nearly to its end)
        t7 = time.perf_counter()
        with open(os.path.join(tmp, 'kept.fastq'), 'rb') as f:
            kept = f.read()
        with open(os.path.join(tmp, 'fallback.fastq'), 'rb') as f:
            fb = f.read()
        assert kept.startswith(fb) or r['hits'][0].file_pos < 400, 'the fallback wrote other records'
    nh = len(r['hits'])
    per = (t5 - t4) / max(k, 1)
    out.append('(b) extract_hits on %d reads x 150 bp as one gzip member (%.0f MB text), scanned with inflate=\'device_any\', records on'
               % (args.gz_reads, len(text) / 1e6))
    out.append('    findseqs (records on): %.3f s; %d hits' % (t1 - t0, nh))
    out.append('    extract_hits from the kept records: %.4f s for all %d hits' % (t3 - t2, nh))
    out.append('    host fallback (Fastq.readrecordat): %.3f s for the first %d hits = %.4f s a hit -> %.1f s for all %d (extrapolated)'
               % (t5 - t4, k, per, per * nh, nh))
    out.append('    (the first hits lie near the head of the file, and a hit costs the inflate of the file up to it: the last hit,'
               ' at %.0f %% of the text, took %.3f s -- about %.0f s for all %d at half that on average)'
               % (100.0 * r['hits'][-1].file_pos / len(text), t7 - t6, (t7 - t6) / 2 * nh, nh))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--gz-reads', type=int, default=1_000_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'records_rate.txt'))
    ap.add_argument('--parts', default='ab')
    args = ap.parse_args()
    out = ['# tools/records_rate.py --reads %d --reps %d --gz-reads %d' % (args.reads, args.reps, args.gz_reads)]
    if 'a' in args.parts:
        part_a(args, out)
        print('\n'.join(out), flush=True)
    if 'b' in args.parts:
        part_b(args, out)
    text = '\n'.join(out) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
