#!/usr/bin/env python3
"""What profiling the input during the scan costs (Scanner(profile=...), findseqs(profile=...)),
written to profiles/profile_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with the profile off and on at 0, 1 and 8 cutoffs, alternately, --reps steps each after two warm-ups:
     the step (scan to finish, wall), the GPU time of the batch's kernels, and kvq_profile_records alone -- as the
     library picks the form of its byte histograms, and in both forms (KVQ_PROFILE_HIST=wave: counted in the wave first;
     =spread: copies spread over the lanes; a child process each) at 0, 1, 4 and 8 cutoffs.  The yardstick is a scan of
     the same text with an EMPTY table -- the record index plus kvq_trim_records, the pass of the same kind the engine
     already had -- on this build and, with --yardstick-parent MS, on the parent's (measured the same way with the
     parent's library).
 (b) profile.profile() of a --gz-reads .fastq.gz against a plain findseqs of it.
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
CUTS8 = '.!5?DIJ~'
FORM_NCUT = (0, 1, 4, 8)


def resident(L, n, rl=150):
    rb = synth.record_bytes(rl)
    g = synth.genome()
    d_genome = scan.DeviceBuffer(g.nbytes); d_genome.upload(g)
    d_data = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_data.ptr, 0, n, rl, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    return g, d_genome, d_data, analytic_chunk_offsets(n, rb, rl), n * rb


def steps(L, scanners, d_data, nbytes, offs, reps):
    """name -> medians of (step ms, batch kernels ms, profile kernel ms), the scanners in turn"""
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
                res[k].append(((t1 - t0) * 1e3, r['kernel_ms'], r.get('profile_kernel_ms', 0.0)))
    return {k: [statistics.median(x[i] for x in v) for i in range(3)] for k, v in res.items()}


def yardstick(L, d_data, nbytes, offs, reps):
    t = scan.Table([], **CFG)
    s = scan.Scanner(t)
    med = steps(L, {'y': s}, d_data, nbytes, offs, reps)['y']
    s.close(); t.close()
    return med[1]


def part_a(args, out):
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    if args.parts == 'y':
        print('yardstick_kernel_ms=%.4f' % yardstick(L, d_data, nbytes, offs, args.reps))
        return
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    modes = {'off': None, 'ncut 0': '', 'ncut 1': '.', 'ncut 8': CUTS8}
    if args.parts == 's':                                   # a child: one form of the histograms, profile kernel alone
        sc = {k: scan.Scanner(t, profile=CUTS8[:k]) for k in FORM_NCUT}
        med = steps(L, sc, d_data, nbytes, offs, args.reps)
        print('form ' + ' '.join('%.4f' % med[k][2] for k in sc))
        return
    sc = {k: scan.Scanner(t, profile=v) for k, v in modes.items()}
    med = steps(L, sc, d_data, nbytes, offs, args.reps)
    for s in sc.values():
        s.close()
    t.close()
    y = yardstick(L, d_data, nbytes, offs, args.reps)
    d_data.free(); d_genome.free()
    forms = {}
    for form in ('wave', 'spread'):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--parts', 's', '--reads', str(args.reads), '--reps', str(args.reps)],
                               env=dict(os.environ, KVQ_PROFILE_HIST=form), stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if child.returncode == 0 and 'form ' in child.stdout:
            forms[form] = [float(x) for x in child.stdout.split('form ')[1].split()]
    out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
               % (args.reads, nbytes / 1e9, args.reps))
    out.append('    profile   step ms   batch kernels ms   kvq_profile_records ms (GB/s of text)')
    for k in modes:
        out.append('    %-7s   %7.3f   %16.3f   %8.3f %s' % (k, med[k][0], med[k][1], med[k][2],
                                                         '(%.0f)' % (nbytes / 1e6 / med[k][2]) if med[k][2] else ''))
    out.append('    kvq_profile_records alone in each form of its byte histograms, ms at ncut ' + ' / '.join(map(str, FORM_NCUT)) + ':')
    for form, what in (('wave', 'counted in the wave first'), ('spread', '8 copies spread over the lanes')):
        if form in forms:
            out.append('      %-32s %s' % (what, ' / '.join('%.3f' % x for x in forms[form])))
    out.append('    yardstick, a scan with an empty table (record index + kvq_trim_records), batch kernels: %.3f ms on this build%s'
               % (y, ', %.3f ms on the parent build' % args.yardstick_parent if args.yardstick_parent else ''))
    yy = args.yardstick_parent or y
    for k in ('ncut 0', 'ncut 1', 'ncut 8'):
        out.append('    %s: pass (batch kernels on - off, the index of a seeded batch and its host round trip included) %.3f ms = %.2fx the yardstick;'
                   ' kernel alone %.2fx; step %+.1f %%' % (k, med[k][1] - med['off'][1], (med[k][1] - med['off'][1]) / yy, med[k][2] / yy,
                                                         100 * (med[k][0] / med['off'][0] - 1)))


def part_b(args, out):
    from kvarq_amd import profile as P
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g, 'MTBC'))
    text = synth.reads(g, 0, args.gz_reads, 150).tobytes()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'reads.fastq.gz')
        with open(path, 'wb') as f:
            f.write(gzip.compress(text, 1, mtime=0))
        engine.config(**dict(CFG, nthreads=8))
        ts = {'findseqs': [], 'findseqs profile=True': [], 'profile.profile()': []}
        for rep in range(4):
            t0 = time.perf_counter(); engine.findseqs(path, seqs); t1 = time.perf_counter()
            r = engine.findseqs(path, seqs, profile=True); t2 = time.perf_counter()
            p = P.profile(path); t3 = time.perf_counter()
            assert p == r['profile'] and p.records == args.gz_reads
            if rep:
                for k, v in zip(ts, (t1 - t0, t2 - t1, t3 - t2)):
                    ts[k].append(v)
    out.append('(b) %d reads x 150 bp as one gzip member (%.0f MB text), host inflate, medians of 3 calls after one warm-up'
               % (args.gz_reads, len(text) / 1e6))
    for k, v in ts.items():
        out.append('    %-22s %.3f s' % (k, statistics.median(v)))
    out.append('    ' + p.summary().replace('\n', '\n    '))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--gz-reads', type=int, default=1_000_000)
    ap.add_argument('--yardstick-parent', type=float, default=0.0, help='the yardstick (--parts y) measured on the parent build, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'profile_rate.txt'))
    ap.add_argument('--parts', default='ab', help="ab, a, b; y: the yardstick alone; s: the spread form alone (both print, neither writes)")
    args = ap.parse_args()
    out = ['# tools/profile_rate.py --reads %d --reps %d --gz-reads %d' % (args.reads, args.reps, args.gz_reads)]
    if 'a' in args.parts or args.parts in ('y', 's'):
        part_a(args, out)
        if args.parts in ('y', 's'):
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
