#!/usr/bin/env python3
"""What the overrepresented sequences cost (Scanner(overrepresented=True)), written to
profiles/over_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with neither, with the duplication alone and with the overrepresented sequences alone, alternately, --reps
     steps each after two warm-ups: the step (scan to finish, wall), the GPU time of the batch's kernels, kvq_profile_records
     alone, kvq_reads_records with the table's settle kernels alone, and kvq_over_records alone.
     The yardstick is the duplication alone (Scanner(duplication=True), kvq_scan_reads_kernel_ms): on this build and, with
     --yardstick-parent MS, on the parent's (``--parts y`` run with the parent's tree prints it: it needs no new symbol).
     The condition, stated before the run: kvq_over_records takes no longer than the yardstick.
 (b) the overrepresented sequences on a text of one record repeated (the contention case): no condition.
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
KEYS = ('kernel_ms', 'profile_kernel_ms', 'reads_kernel_ms', 'over_kernel_ms')


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
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'over_rate.txt'))
    ap.add_argument('--parts', default='ab', help='ab, a, b; y: the yardstick alone (prints, does not write)')
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    if args.parts == 'y':
        s = scan.Scanner(t, duplication=True)
        print('yardstick_kernel_ms=%.4f' % steps(L, {'y': s}, d_data, nbytes, offs, args.reps)['y'][0][3])
        return
    out = ['# tools/over_rate.py --reads %d --reps %d' % (args.reads, args.reps)]

    def line(name, m):
        return '    %-28s %7.3f   %16.3f   %22.3f   %28.3f   %19.3f %s' % (name, m[0], m[1], m[2], m[3], m[4], '(%.0f)' % (nbytes / 1e6 / m[4]) if m[4] else '')

    def what(p):
        o = p.over_info
        top = p.overrepresented[0] if p.overrepresented else None
        return ('%d candidates among the first %d records, %d of %d keyed reads counted on them, %d listed%s'
                % (o['candidates'], o['records_limit'], o['counted'], o['keyed'], o['listed'], ', the first with %d reads' % top.count if top else ''))

    head = '    %-28s step ms   batch kernels ms   kvq_profile_records ms   kvq_reads_records + settle ms   kvq_over_records ms (GB/s of text)' % ''
    if 'a' in args.parts:
        sc = {'off': scan.Scanner(t), 'profile + duplication': scan.Scanner(t, duplication=True), 'profile + overrepresented': scan.Scanner(t, overrepresented=True)}
        med = steps(L, sc, d_data, nbytes, offs, args.reps)
        for s in sc.values():
            s.close()
        out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
                   % (args.reads, nbytes / 1e9, args.reps))
        out.append(head)
        out += [line(k, med[k][0]) for k in sc]
        y = med['profile + duplication'][0][3]
        yy = args.yardstick_parent or y
        r = med['profile + overrepresented'][0][4]
        out.append('    yardstick, the duplication alone (kvq_reads_records with insert, kvq_dup_plan, kvq_dup_purge): %.3f ms on this build%s'
                   % (y, ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
        out.append('    kvq_over_records: %.3f ms = %.2fx the yardstick (the condition: at most 1.00x)' % (r, r / yy))
        out.append('    ' + what(med['profile + overrepresented'][1]['profile']))
    if 'b' in args.parts:
        rb = synth.record_bytes(150)
        one = np.frombuffer(synth.reads(g, 0, 1, 150).tobytes(), dtype=np.uint8)
        assert one.nbytes == rb
        d_one = scan.DeviceBuffer(nbytes)
        d_one.upload(np.tile(one, args.reads))
        s = scan.Scanner(t, overrepresented=True)
        m, r = steps(L, {'o': s}, d_one, nbytes, offs, args.reps)['o']
        out.append('(b) one record repeated %d times (the contention case; no condition)' % args.reads)
        out.append(head)
        out.append(line('profile + overrepresented', m))
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
