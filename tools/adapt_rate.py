#!/usr/bin/env python3
"""What the adapter content costs (Scanner(adapters=...)), written to profiles/adapt_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with neither, with the per-read distributions alone and with the adapter content alone (the default probes:
     adapters=True), alternately, --reps steps each after two warm-ups: the step (scan to finish, wall), the GPU time of the
     batch's kernels, kvq_profile_records alone, kvq_reads_records alone, and kvq_adapt_records alone.
     The yardstick is the per-read distributions alone (Scanner(per_read=True), kvq_scan_reads_kernel_ms): on this build and,
     with --yardstick-parent MS, on the parent's (``--parts y`` run with the parent's tree prints it: it needs no new symbol).
     The condition, stated before the run: kvq_adapt_records takes at most 2 x the yardstick.
 (b) eight probes of 32 bases on the same text: no condition.
 (c) the default probes on a text of one record repeated that holds an adapter at cycle 100 (the contention case for one
     ``first`` bin): no condition.
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
KEYS = ('kernel_ms', 'profile_kernel_ms', 'reads_kernel_ms', 'adapt_kernel_ms')
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


def eight_probes():
    rng = np.random.RandomState(18)
    return [rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), 32).tobytes() for _ in range(8)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adapt_rate.txt'))
    ap.add_argument('--parts', default='abc', help='any of a, b, c; y: the yardstick alone (prints, does not write)')
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    if args.parts == 'y':
        s = scan.Scanner(t, per_read=True)
        print('yardstick_kernel_ms=%.4f' % steps(L, {'y': s}, d_data, nbytes, offs, args.reps)['y'][0][3])
        return
    out = ['# tools/adapt_rate.py --reads %d --reps %d' % (args.reads, args.reps)]

    def line(name, m):
        return '    %-28s %7.3f   %16.3f   %22.3f   %20.3f   %20.3f %s' % (name, m[0], m[1], m[2], m[3], m[4], '(%.0f)' % (nbytes / 1e6 / m[4]) if m[4] else '')

    def what(p):
        a = p.adapters
        return ('%d probes of %s bases: %d of %d reads with a full occurrence, %d more with a tail only; clipped length Q10 %g, Q50 %g'
                % (len(a.names), sorted(set(a.lengths)), a.with_adapter, a.records, a.tail_only, p.clip_quantile(0.1), p.clip_quantile(0.5)))

    head = '    %-28s step ms   batch kernels ms   kvq_profile_records ms   kvq_reads_records ms   kvq_adapt_records ms (GB/s of text)' % ''
    if 'a' in args.parts:
        sc = {'off': scan.Scanner(t), 'profile + per-read': scan.Scanner(t, per_read=True), 'profile + adapters': scan.Scanner(t, adapters=True)}
        med = steps(L, sc, d_data, nbytes, offs, args.reps)
        for s in sc.values():
            s.close()
        out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
                   % (args.reads, nbytes / 1e9, args.reps))
        out.append(head)
        out += [line(k, med[k][0]) for k in sc]
        y = med['profile + per-read'][0][3]
        yy = args.yardstick_parent or y
        r = med['profile + adapters'][0][4]
        out.append('    yardstick, the per-read distributions alone (kvq_reads_records): %.3f ms on this build%s'
                   % (y, ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
        out.append('    kvq_adapt_records: %.3f ms = %.2fx the yardstick (the condition: at most 2.00x)' % (r, r / yy))
        out.append('    ' + what(med['profile + adapters'][1]['profile']))
    if 'b' in args.parts:
        s = scan.Scanner(t, adapters=eight_probes())
        m, r = steps(L, {'e': s}, d_data, nbytes, offs, args.reps)['e']
        out.append('(b) eight probes of 32 bases on the same text (no condition)')
        out.append(head)
        out.append(line('profile + adapters', m))
        out.append('    ' + what(r['profile']))
        s.close()
    if 'c' in args.parts:
        rb = synth.record_bytes(150)
        one = np.frombuffer(synth.reads(g, 0, 1, 150).tobytes(), dtype=np.uint8).copy()
        assert one.nbytes == rb
        at = one.tobytes().index(b'\n') + 1 + 100
        one[at:at + len(ADAPTER)] = np.frombuffer(ADAPTER, dtype=np.uint8)
        d_one = scan.DeviceBuffer(nbytes)
        d_one.upload(np.tile(one, args.reads))
        s = scan.Scanner(t, adapters=True)
        m, r = steps(L, {'c': s}, d_one, nbytes, offs, args.reps)['c']
        out.append('(c) one record repeated %d times, an adapter at cycle 100 (the contention case for one bin; no condition)' % args.reads)
        out.append(head)
        out.append(line('profile + adapters', m))
        out.append('    ' + what(r['profile']))
        s.close(); d_one.free()
    t.close()
    d_data.free(); d_genome.free()
    text = '\n'.join(out) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
