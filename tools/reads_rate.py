#!/usr/bin/env python3
"""What the per-read distributions and the duplication cost (Scanner(per_read=True, duplication=True)),
written to profiles/reads_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with neither, with the profile at zero cutoffs, with the per-read distributions added, and with the
     duplication added to those, alternately, --reps steps each after two warm-ups: the step (scan to finish, wall), the GPU
     time of the batch's kernels, kvq_profile_records alone, and kvq_reads_records with the table's settle kernels alone.
     The yardstick is kvq_profile_records at zero cutoffs: on this build and, with --yardstick-parent MS, on the parent's
     (``--parts y`` run with the parent's tree prints it: it needs no new symbol).  The condition, stated before the run:
     kvq_reads_records alone, without the duplication, takes no longer than the yardstick.
 (b) the duplication alone on that text (nearly every key distinct: the level it reaches is reported) and on a text of one
     key repeated (the contention case): kvq_reads_records with insert and settle, ms and GB/s of text.
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
KEYS = ('kernel_ms', 'profile_kernel_ms', 'reads_kernel_ms')


def resident(L, n, rl=150):
    rb = synth.record_bytes(rl)
    g = synth.genome()
    d_genome = scan.DeviceBuffer(g.nbytes); d_genome.upload(g)
    d_data = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_data.ptr, 0, n, rl, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    return g, d_genome, d_data, analytic_chunk_offsets(n, rb, rl), n * rb


def steps(L, scanners, d_data, nbytes, offs, reps):
    """name -> (medians of step ms, batch kernels ms, profile kernel ms, reads kernels ms; the last result), the scanners in turn"""
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
    return {k: ([statistics.median(x[i] for x in v) for i in range(4)], last[k]) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reads_rate.txt'))
    ap.add_argument('--parts', default='ab', help='ab, a, b; y: the yardstick alone (prints, does not write)')
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    if args.parts == 'y':
        s = scan.Scanner(t, profile='')
        print('yardstick_kernel_ms=%.4f' % steps(L, {'y': s}, d_data, nbytes, offs, args.reps)['y'][0][2])
        return
    out = ['# tools/reads_rate.py --reads %d --reps %d' % (args.reads, args.reps)]
    if 'a' in args.parts:
        sc = {'off': scan.Scanner(t), 'profile, ncut 0': scan.Scanner(t, profile=''), 'profile + per-read': scan.Scanner(t, per_read=True),
              'profile + per-read + duplication': scan.Scanner(t, per_read=True, duplication=True)}
        med = steps(L, sc, d_data, nbytes, offs, args.reps)
        for s in sc.values():
            s.close()
        out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
                   % (args.reads, nbytes / 1e9, args.reps))
        out.append('    %-34s step ms   batch kernels ms   kvq_profile_records ms   kvq_reads_records + settle ms (GB/s of text)' % '')
        for k in sc:
            m = med[k][0]
            out.append('    %-34s %7.3f   %16.3f   %22.3f   %8.3f %s' % (k, m[0], m[1], m[2], m[3], '(%.0f)' % (nbytes / 1e6 / m[3]) if m[3] else ''))
        y = med['profile, ncut 0'][0][2]
        yy = args.yardstick_parent or y
        r = med['profile + per-read'][0][3]
        out.append('    yardstick, kvq_profile_records at zero cutoffs: %.3f ms on this build%s'
                   % (y, ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
        out.append('    kvq_reads_records alone, without the duplication: %.3f ms = %.2fx the yardstick (the condition: at most 1.00x)' % (r, r / yy))
        p = med['profile + per-read + duplication'][1]['profile']
        out.append('    ' + '\n    '.join(p.per_read_lines(dQ=0)[:1] + p.duplication_lines()[:1]))
    if 'b' in args.parts:
        rb = synth.record_bytes(150)
        one = np.frombuffer(synth.reads(g, 0, 1, 150).tobytes(), dtype=np.uint8)
        assert one.nbytes == rb
        d_one = scan.DeviceBuffer(nbytes)
        d_one.upload(np.tile(one, args.reads))
        s = scan.Scanner(t, duplication=True)
        out.append('(b) the duplication alone (Scanner(duplication=True)): kvq_reads_records with insert, kvq_dup_plan and kvq_dup_purge behind every slice, ms (GB/s of text)')
        for name, d in (('the bench text', d_data), ('one record repeated', d_one)):
            m, r = steps(L, {'d': s}, d, nbytes, offs, args.reps)['d']
            dd = r['profile'].duplication
            out.append('    %-20s %8.3f (%.0f)   level %d, %d keys tracked of %d reads keyed, duplicate share %.4f'
                       % (name, m[3], nbytes / 1e6 / m[3], dd['level'], dd['tracked_distinct'], dd['keyed'], r['profile'].duplicate_share()))
        s.close(); d_one.free()
    t.close()
    d_data.free(); d_genome.free()
    text = '\n'.join(out) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
