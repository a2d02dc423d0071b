#!/usr/bin/env python3
"""What the read-list route does for long reads (Scanner(long_reads=True), findseqs(long_reads=True)),
written to profiles/long_rate.txt:
 (a) --reads reads x --length bases cut from synth.genome() (every score good: the trim keeps the whole read), resident in
     HBM, the MTBC-shaped table, the product config, through scan.Scanner: the default route -- the yardstick: the scan
     kernel's pass, rolled back, and the whole-batch exhaustive redo -- and the read-list route, alternately, --reps steps
     each after two warm-ups: the step (scan to finish, wall), the GPU time of all kernels of the batch, kvq_seed_list alone.
     The front end both routes share (index_records + kvq_trim_records) is the batch of a scan with an empty table.
     The condition: all kernels of the batch on the route take at most 1/10 of the yardstick's.  With --yardstick-parent MS
     the yardstick is the one measured on the parent's tree (``--parts y`` runs there: it names no new option).
 (b) bench.py's 150-base text (--short-reads reads) through both routes: how far the route is from kvq_scan_bp there.
 (c) --bam-reads of the long reads as an unaligned BAM, engine.findseqs end to end with and without the option.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from kvarq_amd import _lib, engine, scan, synth  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402

CFG = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')      # kvarq/config.py:2-10
NAME = 13                                                               # bytes of a read's name: 'L.' and eleven digits


def long_text(g, n, length, first=0):
    """n records '@L.<11 digits>', `length` bases cut from the genome at evenly drawn places, '+', scores of 'I'"""
    rb = 1 + NAME + 1 + length + 3 + length + 1
    out = np.empty((n, rb), np.uint8)
    with np.errstate(over='ignore'):
        start = (synth.mix64(np.arange(first, first + n, dtype=np.uint64) + np.uint64(synth.SEED)) % np.uint64(len(g) - length + 1)).astype(np.int64)
    out[:, 0] = ord('@')
    out[:, 1:1 + NAME] = np.frombuffer(b''.join(b'L.%011d' % r for r in range(first, first + n)), np.uint8).reshape(n, NAME)
    out[:, 1 + NAME] = 10
    for r in range(n):
        out[r, 2 + NAME:2 + NAME + length] = g[start[r]:start[r] + length]
    out[:, 2 + NAME + length:5 + NAME + length] = np.frombuffer(b'\n+\n', np.uint8)
    out[:, 5 + NAME + length:5 + NAME + 2 * length] = ord('I')
    out[:, rb - 1] = 10
    return out.reshape(-1)


def steps(L, scanners, d_ptr, nbytes, offs, reps):
    """name -> medians of (step ms, batch kernels ms, main kernel ms), the scanners in turn, and each one's last result"""
    res, last = {k: [] for k in scanners}, {}
    for rep in range(reps + 2):
        for k, s in scanners.items():
            s.reset()
            L.kvq_device_synchronize()
            t0 = time.perf_counter()
            s.scan_device(d_ptr, nbytes, offs)
            r = s.finish(hits=False, stats=rep == 0)
            t1 = time.perf_counter()
            if rep == 0:
                last[k] = r
            if rep >= 2:
                res[k].append([(t1 - t0) * 1e3, r['kernel_ms'], r['main_kernel_ms']])
    return {k: [statistics.median(x[i] for x in v) for i in range(3)] for k, v in res.items()}, last


def part_a(args, out, g, seqs):
    L = _lib.lib()
    text = long_text(g, args.reads, args.length)
    offs = scan.chunk_offsets(text)
    d = scan.DeviceBuffer(text.nbytes); d.upload(text)
    t = scan.Table(seqs, **CFG)
    if args.parts == 'y':                                   # the yardstick alone: runs with the parent's tree as well
        med, last = steps(L, {'y': scan.Scanner(t)}, d.ptr, text.nbytes, offs, args.reps)
        print('yardstick_kernel_ms=%.4f step_ms=%.4f hits=%d path=%s' % (med['y'][1], med['y'][0], last['y']['n_hits'], last['y']['path']))
        return
    empty = scan.Table([], **CFG)
    sc = {'default route': scan.Scanner(t), 'read list': scan.Scanner(t, long_reads=True), 'front end (empty table)': scan.Scanner(empty)}
    med, last = steps(L, sc, d.ptr, text.nbytes, offs, args.reps)
    a, b = last['default route'], last['read list']
    assert a['n_hits'] == b['n_hits'] and (a['counters'] == b['counters']).all(), 'the routes disagree'
    assert b['path']['read_list'] and not b['path']['seeded'], (a['path'], b['path'])
    how = ', '.join(k for k, v in a['path'].items() if v)
    for s in sc.values():
        s.close()
    t.close(); empty.close(); d.free()
    out.append('(a) %d reads x %d bases resident (%.0f MB), MTBC table (%d sequences), product config; Scanner, one batch; medians of %d steps each, alternating; %d hits either way'
               % (args.reads, args.length, text.nbytes / 1e6, len(seqs), args.reps, b['n_hits']))
    out.append('    %-26s step ms   batch kernels ms   main kernel ms   GB/s of text (batch kernels)' % '')
    for k in sc:
        out.append('    %-26s %7.2f   %16.3f   %14.3f   %6.1f' % (k, med[k][0], med[k][1], med[k][2], text.nbytes / 1e6 / med[k][1]))
    y = args.yardstick_parent or med['default route'][1]
    r = med['read list']
    out.append('    yardstick, all kernels of the batch on the default route (its path: %s): %.3f ms on this build%s'
               % (how, med['default route'][1], ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
    out.append('    read list: all kernels %.3f ms = 1/%.0f of the yardstick (condition: at most 1/10: %s); kvq_seed_list alone %.3f ms, front end alone %.3f ms'
               % (r[1], y / r[1], 'met' if r[1] * 10 <= y else 'NOT met', r[2], med['front end (empty table)'][1]))


def part_b(args, out, g, seqs):
    L = _lib.lib()
    n, rl = args.short_reads, 150
    rb = synth.record_bytes(rl)
    dg = scan.DeviceBuffer(g.nbytes); dg.upload(g)
    d = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d.ptr, 0, n, rl, synth.SEED, dg.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    t = scan.Table(seqs, **CFG)
    sc = {'default route (kvq_scan_bp)': scan.Scanner(t), 'read list': scan.Scanner(t, long_reads=True)}
    med, last = steps(L, sc, d.ptr, n * rb, analytic_chunk_offsets(n, rb, rl), args.reps)
    a, b = last['default route (kvq_scan_bp)'], last['read list']
    assert a['n_hits'] == b['n_hits'] and (a['counters'] == b['counters']).all(), 'the routes disagree'
    for s in sc.values():
        s.close()
    t.close(); d.free(); dg.free()
    out.append('(b) %d reads x 150 bp resident (%.0f MB), the same table and config' % (n, n * rb / 1e6))
    for k in sc:
        out.append('    %-28s step %7.2f ms   batch kernels %8.3f ms   main kernel %8.3f ms   %6.1f GB/s' % (k, med[k][0], med[k][1], med[k][2], n * rb / 1e6 / med[k][1]))


def part_c(args, out, g, seqs):
    from bgzf_rate import write_bgzf
    n, length = args.bam_reads, args.length
    text = long_text(g, n, length).reshape(n, -1)
    name, bases = text[:, 1:1 + NAME], text[:, 2 + NAME:2 + NAME + length]
    lut = np.zeros(256, np.uint8)
    for c, v in zip(b'=ACMGRSVTWYHKDBN', range(16)):
        lut[c] = v
    codes = lut[bases]
    body = 32 + NAME + 1 + length // 2 + length
    fixed = np.frombuffer(np.array([(body, -1, -1, NAME + 1, 255, 4680, 0, 4, length, -1, -1, 0)],
                                   dtype=[('bs', '<i4'), ('ref', '<i4'), ('pos', '<i4'), ('lrn', 'u1'), ('mapq', 'u1'), ('bin', '<u2'), ('ncig', '<u2'),
                                          ('flag', '<u2'), ('lseq', '<i4'), ('nref', '<i4'), ('npos', '<i4'), ('tlen', '<i4')]).tobytes(), np.uint8)
    rec = np.empty((n, 4 + body), np.uint8)
    rec[:, :36] = fixed; rec[:, 36:36 + NAME] = name; rec[:, 36 + NAME] = 0
    rec[:, 37 + NAME:37 + NAME + length // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, 37 + NAME + length // 2:] = ord('I') - 33
    stream = np.concatenate([np.frombuffer(b'BAM\x01' + bytes(8), np.uint8), rec.reshape(-1)])
    with tempfile.TemporaryDirectory() as tmp:
        raw, path = os.path.join(tmp, 'long.raw'), os.path.join(tmp, 'long.bam')
        stream.tofile(raw)
        write_bgzf(path, raw, stream.nbytes, 1, min(16, len(os.sched_getaffinity(0))))
        os.remove(raw)
        engine.config(**dict(CFG, nthreads=16))
        ts, res = {False: [], True: []}, {}
        for rep in range(args.bam_reps + 1):
            for lr in (False, True):
                t0 = time.perf_counter()
                res[lr] = engine.findseqs(path, seqs, long_reads=lr)
                if rep:
                    ts[lr].append(time.perf_counter() - t0)
                assert engine.last_inflate() == 'device_bam' and engine.last_long_reads() is lr
        assert res[False]['hits'] == res[True]['hits'] and res[False]['stats'] == res[True]['stats']
        size = os.path.getsize(path)
    out.append('(c) %d of those reads as an unaligned BAM (%.0f MB, %.0f MB of text), engine.findseqs end to end, medians of %d calls after one warm-up, alternating; %d hits either way'
               % (n, size / 1e6, text.nbytes / 1e6, args.bam_reps, len(res[True]['hits'])))
    for lr in (False, True):
        out.append('    long_reads=%-5s  %.3f s' % (lr, statistics.median(ts[lr])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=20_000)
    ap.add_argument('--length', type=int, default=12_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--short-reads', type=int, default=2_000_000)
    ap.add_argument('--bam-reads', type=int, default=5_000)
    ap.add_argument('--bam-reps', type=int, default=3)
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'long_rate.txt'))
    ap.add_argument('--parts', default='abc', help='any of a, b, c; y: the yardstick alone (prints, does not write)')
    args = ap.parse_args()
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g, 'MTBC'))
    out = ['# tools/long_rate.py --reads %d --length %d --reps %d --short-reads %d --bam-reads %d' % (args.reads, args.length, args.reps, args.short_reads, args.bam_reads)]
    if args.parts == 'y':
        return part_a(args, out, g, seqs)
    for p, f in (('a', part_a), ('b', part_b), ('c', part_c)):
        if p in args.parts:
            f(args, out, g, seqs)
            print('\n'.join(out), flush=True)
    text = '\n'.join(out) + '\n'
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
