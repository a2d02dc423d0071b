#!/usr/bin/env python3
"""What the per-cycle counts cost (Scanner(cycles=True), findseqs(cycles=True)), written to
profiles/cycles_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with neither, with the profile at zero cutoffs, and with the cycles added, alternately, --reps steps each
     after two warm-ups: the step (scan to finish, wall), the GPU time of the batch's kernels, kvq_profile_records alone and
     kvq_profile_cycles alone -- at the slab width the library is built with, and at both widths (KVQ_CYCLES_SLAB=64 / 128,
     a child process each).  The yardstick is kvq_profile_records at zero cutoffs: on this build and, with
     --yardstick-parent MS, on the parent's (``--parts y`` run with the parent's tree prints it: it needs no new symbol).
 (b) profile.profile() of a --gz-reads .fastq.gz with and without cycles=True.
"""
import argparse
import gzip
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvarq_amd import _lib, engine, scan, synth  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402

CFG = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')      # kvarq/config.py:2-10
WIDTHS = (64, 128)
KEYS = ('kernel_ms', 'profile_kernel_ms', 'cycles_kernel_ms')


def resident(L, n, rl=150):
    rb = synth.record_bytes(rl)
    g = synth.genome()
    d_genome = scan.DeviceBuffer(g.nbytes); d_genome.upload(g)
    d_data = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_data.ptr, 0, n, rl, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    return g, d_genome, d_data, analytic_chunk_offsets(n, rb, rl), n * rb


def steps(L, scanners, d_data, nbytes, offs, reps):
    """name -> medians of (step ms, batch kernels ms, profile kernel ms, cycles kernel ms), the scanners in turn"""
    res = {k: [] for k in scanners}
    for rep in range(reps + 2):
        for k, s in scanners.items():
            s.reset()
            L.kvq_device_synchronize()
            t0 = time.perf_counter()
            s.scan_device(d_data.ptr, nbytes, offs)
            r = s.finish(hits=False, stats=False)
            t1 = time.perf_counter()
            if rep >= 2:
                res[k].append([(t1 - t0) * 1e3] + [r.get(key, 0.0) for key in KEYS])
    return {k: [statistics.median(x[i] for x in v) for i in range(4)] for k, v in res.items()}


def part_a(args, out):
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    if args.parts == 'y':                                   # the yardstick alone: runs with the parent's tree as well
        s = scan.Scanner(t, profile='')
        print('yardstick_kernel_ms=%.4f' % steps(L, {'y': s}, d_data, nbytes, offs, args.reps)['y'][2])
        return
    if args.parts == 'w':                                   # a child: one slab width, the cycles kernel alone
        s = scan.Scanner(t, cycles=True)
        print('width %.4f' % steps(L, {'w': s}, d_data, nbytes, offs, args.reps)['w'][3])
        return
    sc = {'off': scan.Scanner(t), 'profile, ncut 0': scan.Scanner(t, profile=''), 'profile + cycles': scan.Scanner(t, cycles=True)}
    med = steps(L, sc, d_data, nbytes, offs, args.reps)
    for s in sc.values():
        s.close()
    t.close()
    d_data.free(); d_genome.free()
    widths = {}
    for w in WIDTHS:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--parts', 'w', '--reads', str(args.reads), '--reps', str(args.reps)],
                               env=dict(os.environ, KVQ_CYCLES_SLAB=str(w)), stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if child.returncode == 0 and 'width ' in child.stdout:
            widths[w] = float(child.stdout.split('width ')[1].split()[0])
    out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
               % (args.reads, nbytes / 1e9, args.reps))
    out.append('    %-18s step ms   batch kernels ms   kvq_profile_records ms   kvq_profile_cycles ms (GB/s of text)' % '')
    for k in sc:
        out.append('    %-18s %7.3f   %16.3f   %22.3f   %8.3f %s' % (k, med[k][0], med[k][1], med[k][2], med[k][3],
                                                                 '(%.0f)' % (nbytes / 1e6 / med[k][3]) if med[k][3] else ''))
    out.append('    kvq_profile_cycles alone at each slab width, ms: ' + ', '.join('W = %d: %.3f' % (w, v) for w, v in widths.items()))
    y = med['profile, ncut 0'][2]
    out.append('    yardstick, kvq_profile_records at zero cutoffs: %.3f ms on this build%s'
               % (y, ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
    yy = args.yardstick_parent or y
    c = med['profile + cycles']
    out.append('    kvq_profile_cycles alone: %.2fx the yardstick (expected: at most 1.25x)%s; the step with the cycles: %+.1f %% over the profile alone'
               % (c[3] / yy, ''.join('; W = %d: %.2fx' % (w, v / yy) for w, v in widths.items()), 100 * (c[0] / med['profile, ncut 0'][0] - 1)))


def part_b(args, out):
    from kvarq_amd import profile as P
    g = synth.genome()
    text = synth.reads(g, 0, args.gz_reads, 150).tobytes()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'reads.fastq.gz')
        with open(path, 'wb') as f:
            f.write(gzip.compress(text, 1, mtime=0))
        engine.config(**dict(CFG, nthreads=8))
        ts = {'profile.profile()': [], 'profile.profile(cycles=True)': []}
        for rep in range(4):
            t0 = time.perf_counter(); p = P.profile(path); t1 = time.perf_counter()
            q = P.profile(path, cycles=True); t2 = time.perf_counter()
            assert (p.words == q.words).all() and q.records == args.gz_reads and q.last_cycle == 149
            if rep:
                for k, v in zip(ts, (t1 - t0, t2 - t1)):
                    ts[k].append(v)
    out.append('(b) %d reads x 150 bp as one gzip member (%.0f MB text), host inflate, medians of 3 calls after one warm-up'
               % (args.gz_reads, len(text) / 1e6))
    for k, v in ts.items():
        out.append('    %-28s %.3f s' % (k, statistics.median(v)))
    out.append('    ' + '\n    '.join(q.cycle_lines(25)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--gz-reads', type=int, default=1_000_000)
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cycles_rate.txt'))
    ap.add_argument('--parts', default='ab', help="ab, a, b; y: the yardstick alone; w: the cycles kernel alone (both print, neither writes)")
    args = ap.parse_args()
    out = ['# tools/cycles_rate.py --reads %d --reps %d --gz-reads %d' % (args.reads, args.reps, args.gz_reads)]
    if 'a' in args.parts or args.parts in ('y', 'w'):
        part_a(args, out)
        if args.parts in ('y', 'w'):
            return
        print('\n'.join(out), flush=True)
    if 'b' in args.parts:
        part_b(args, out)
    text = '\n'.join(out) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
