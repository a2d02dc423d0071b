#!/usr/bin/env python3
"""What the adapter clip costs (Scanner(clip=...)), written to profiles/clip_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with nothing, with the adapter content alone (adapters=True) and with the clip alone (clip=True: the same
     probes), alternately, --reps steps each after two warm-ups: the step (scan to finish, wall), the GPU time of the batch's
     kernels, kvq_adapt_records alone and kvq_clip_records alone.
     The yardstick is kvq_adapt_records<4> ON THE PARENT BUILD (``--parts p`` run with the parent's tree prints it: it needs no
     new symbol; hand it over with --adapt-parent MS).  The condition, stated before the run: kvq_clip_records<4> takes at most
     1.25 x that.  The step with the clip on -- index, clip and scan, the host round trip of the index among them -- is reported
     without a condition.
 (b) the default probes on a text of one record repeated that holds an adapter at cycle 100, where every record stores: no
     condition.
The clip WRITES the resident text: from the first step with it on, the text is MASK(text) for every scanner (the few reads of
the synthetic text that match lose the scores behind their match).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from kvarq_amd import _lib, scan, synth  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402

CFG = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')      # kvarq/config.py:2-10
KEYS = ('kernel_ms', 'main_kernel_ms', 'adapt_kernel_ms', 'clip_kernel_ms')
ADAPTER = b'AGATCGGAAGAG'


def resident(L, n, rl=150):
    rb = synth.record_bytes(rl)
    g = synth.genome()
    d_genome = scan.DeviceBuffer(g.nbytes); d_genome.upload(g)
    d_data = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_data.ptr, 0, n, rl, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    return g, d_genome, d_data, analytic_chunk_offsets(n, rb, rl), n * rb


def steps(L, scanners, d_data, nbytes, offs, reps):
    """name -> (medians of step ms and of KEYS; the last result), the scanners in turn"""
    res, last = {k: [] for k in scanners}, {}
    for rep in range(reps + 2):
        for k, s in scanners.items():
            s.reset()
            L.kvq_device_synchronize()
            t0 = time.perf_counter()
            s.scan_device(d_data.ptr, nbytes, offs)
            r = s.finish(hits=False, stats=False)
            t1 = time.perf_counter()
            last[k] = r
            if rep >= 2:
                res[k].append([(t1 - t0) * 1e3] + [r.get(key, 0.0) for key in KEYS])
    return {k: ([statistics.median(x[i] for x in v) for i in range(1 + len(KEYS))], last[k]) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--adapt-parent', type=float, default=0.0, help='kvq_adapt_records<4> (--parts p) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_rate.txt'))
    ap.add_argument('--parts', default='ab', help='any of a, b; p: kvq_adapt_records alone (prints, does not write)')
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    if args.parts == 'p':
        s = scan.Scanner(t, adapters=True)
        print('adapt_kernel_ms=%.4f' % steps(L, {'p': s}, d_data, nbytes, offs, args.reps)['p'][0][3])
        return
    out = ['# tools/clip_rate.py --reads %d --reps %d' % (args.reads, args.reps)]
    head = '    %-22s step ms   batch kernels ms   scan kernel ms   kvq_adapt_records ms   kvq_clip_records ms (GB/s of text)' % ''

    def line(name, m):
        return '    %-22s %7.3f   %16.3f   %14.3f   %20.3f   %19.3f %s' % (name, m[0], m[1], m[2], m[3], m[4], '(%.0f)' % (nbytes / 1e6 / m[4]) if m[4] else '')

    def what(r):
        c = r['clip']
        return '%d probes: %d of %d records clipped, %d score positions masked, %d bases cut' % (len(c.probes), c.clipped, c.records, c.masked, c.bases_cut)

    if 'a' in args.parts:
        sc = {'off': scan.Scanner(t), 'profile + adapters': scan.Scanner(t, adapters=True), 'clip': scan.Scanner(t, clip=True)}
        med = steps(L, sc, d_data, nbytes, offs, args.reps)
        for s in sc.values():
            s.close()
        out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
                   % (args.reads, nbytes / 1e9, args.reps))
        out.append(head)
        out += [line(k, med[k][0]) for k in sc]
        a, c = med['profile + adapters'][0][3], med['clip'][0][4]
        y = args.adapt_parent or a
        out.append('    yardstick, kvq_adapt_records<4>: %.3f ms on this build%s' % (a, ', %.3f ms on the parent build' % args.adapt_parent if args.adapt_parent else ''))
        out.append('    kvq_clip_records<4>: %.3f ms = %.2fx the yardstick (the condition: at most 1.25x)' % (c, c / y))
        out.append('    the step with the clip on (index, clip, scan): %.3f ms, against %.3f ms with it off' % (med['clip'][0][0], med['off'][0][0]))
        out.append('    ' + what(med['clip'][1]))
    if 'b' in args.parts:
        rb = synth.record_bytes(150)
        one = np.frombuffer(synth.reads(g, 0, 1, 150).tobytes(), dtype=np.uint8).copy()
        assert one.nbytes == rb
        at = one.tobytes().index(b'\n') + 1 + 100
        one[at:at + len(ADAPTER)] = np.frombuffer(ADAPTER, dtype=np.uint8)
        d_one = scan.DeviceBuffer(nbytes)
        d_one.upload(np.tile(one, args.reads))
        s = scan.Scanner(t, clip=True)
        m, r = steps(L, {'b': s}, d_one, nbytes, offs, args.reps)['b']
        out.append('(b) one record repeated %d times, an adapter at cycle 100: every record stores (no condition)' % args.reads)
        out.append(head)
        out.append(line('clip', m))
        out.append('    ' + what(r))
        s.close(); d_one.free()
    t.close()
    d_data.free(); d_genome.free()
    text = '\n'.join(out) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
