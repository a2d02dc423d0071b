#!/usr/bin/env python3
"""What adapter probes that tolerate mismatches cost and find (adapter_mismatches=), written to
profiles/adapt_mm_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through scan.Scanner
     with the adapter content and with the clip, each exact and at per = 10 (the known adapters: four 12-base probes),
     alternately, --reps steps each after two warm-ups: kvq_adapt_records<4> / kvq_adapt_records_mm<4> alone and
     kvq_clip_records<4> / kvq_clip_records_mm<4> alone.
     The yardsticks are the two exact kernels ON THE PARENT BUILD, measured in the same session (the parent's tools/clip_rate.py
     prints both; hand them over with --adapt-parent MS --clip-parent MS).  The conditions, stated before the run: each tolerant
     kernel takes at most 2.5 x its yardstick -- the inner loop counts about 16 x (3 + 4 x 6) operations a lane and round against
     about 16 x (2 + 4 x 2) for the pre-test, 2.3 x, everything else shared; the margin covers the lost early-out.
 (b) without a condition: --noisy-reads reads that hold the universal adapter from cycle 100 on, each adapter base substituted
     with probability 2 %: the clipped share exact and at per = 10 (the arithmetic says 78 % and 98 %).
Part (c) of the file -- bench.py with the option off, the parent's tree and this one alternating three times -- is no work of this
tool: it is appended from those runs.
The clip WRITES the resident text: from the first step with it on, the text is MASK(text) for every scanner.
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
from tools.clip_rate import CFG, resident  # noqa: E402

UNIVERSAL = b'AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCACGATCTCGTATGC'[:50]  # 50 bases: cycles 100 .. 149
BOUND = 2.5


def steps(L, scanners, d_data, nbytes, offs, reps):
    """name -> (median step ms, median adapt kernel ms, median clip kernel ms, the last result), the scanners in turn"""
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
                res[k].append(((t1 - t0) * 1e3, r.get('adapt_kernel_ms', 0.0), r.get('clip_kernel_ms', 0.0)))
    return {k: tuple(statistics.median(x[i] for x in v) for i in range(3)) + (last[k],) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--noisy-reads', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--adapt-parent', type=float, default=0.0, help='kvq_adapt_records<4> measured on the parent build in this session, ms')
    ap.add_argument('--clip-parent', type=float, default=0.0, help='kvq_clip_records<4> measured on the parent build in this session, ms')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adapt_mm_rate.txt'))
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    out = ['# tools/adapt_mm_rate.py --reads %d --noisy-reads %d --reps %d' % (args.reads, args.noisy_reads, args.reps)]
    sc = {'adapters exact': scan.Scanner(t, adapters=True), 'adapters per=10': scan.Scanner(t, adapters=True, adapter_mismatches=10),
          'clip exact': scan.Scanner(t, clip=True), 'clip per=10': scan.Scanner(t, clip=True, adapter_mismatches=10)}
    med = steps(L, sc, d_data, nbytes, offs, args.reps)
    for s in sc.values():
        s.close()
    out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config, the four known 12-base probes; Scanner, one batch; medians of %d steps each, alternating'
               % (args.reads, nbytes / 1e9, args.reps))
    out.append('    %-18s step ms   adapt kernel ms   clip kernel ms' % '')
    out += ['    %-18s %7.3f   %15.3f   %14.3f' % ((k,) + med[k][:3]) for k in sc]
    for what, exact, mm, parent in (('kvq_adapt_records_mm<4>', med['adapters exact'][1], med['adapters per=10'][1], args.adapt_parent),
                                    ('kvq_clip_records_mm<4>', med['clip exact'][2], med['clip per=10'][2], args.clip_parent)):
        y = parent or exact
        out.append('    %s: %.3f ms; the exact kernel %.3f ms on this build%s; %.2fx the yardstick (the condition: at most %.1fx): %s'
                   % (what, mm, exact, ', %.3f ms on the parent build' % parent if parent else ' (no parent figure given: this build is the yardstick)',
                      mm / y, BOUND, 'HOLDS' if mm <= BOUND * y else 'FAILS'))
    a0, a1 = med['adapters exact'][3]['profile'], med['adapters per=10'][3]['profile']
    out.append('    clipped share of the synthetic reads: %.4f %% exact, %.4f %% at per = 10' % (100 * a0.clipped_share(), 100 * a1.clipped_share()))
    print('\n'.join(out), flush=True)
    d_data.free()
    # (b) the universal adapter from cycle 100 on, 2 % substitutions
    n, rb = args.noisy_reads, synth.record_bytes(150)
    d_noisy = scan.DeviceBuffer(n * rb)
    if L.kvq_synth_reads_device(d_noisy.ptr, 0, n, 150, synth.SEED, d_genome.ptr, g.nbytes):
        raise SystemExit('synthetic generator failed: %s' % (_lib.last_error(),))
    recs = d_noisy.download(n * rb).reshape(n, rb)
    at = recs[0].tobytes().index(b'\n') + 1 + 100
    rng = np.random.RandomState(20)
    ada = np.tile(np.frombuffer(UNIVERSAL, dtype=np.uint8), (n, 1))
    hit = rng.random_sample(ada.shape) < 0.02
    other = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.randint(0, 4, ada.shape)]
    other = np.where(other == ada, np.frombuffer(b'CGTA', dtype=np.uint8)[rng.randint(0, 4, ada.shape)], other)
    hit &= other != ada
    recs[:, at:at + 50] = np.where(hit, other, ada)
    d_noisy.upload(recs.reshape(-1))
    noffs = analytic_chunk_offsets(n, rb, 150)
    shares = {}
    for name, kw in (('exact', {}), ('per=10', dict(adapter_mismatches=10))):
        s = scan.Scanner(t, adapters=True, **kw)
        s.scan_device(d_noisy.ptr, n * rb, noffs)
        p = s.finish(hits=False, stats=False)['profile']
        shares[name] = (p.clipped_share(), p.adapters.first_mismatches[0].tolist())
        s.close()
    out.append('(b) %d reads x 150 bp, the universal adapter from cycle 100 on, %.2f %% of its bases substituted (no condition; the arithmetic: 78 %% and 98 %%)'
               % (n, 100.0 * hit.mean()))
    out.append('    clipped share: %.2f %% exact, %.2f %% at per = 10 (first occurrences of the universal probe with 0/1 mismatches: %d/%d)'
               % (100 * shares['exact'][0], 100 * shares['per=10'][0], shares['per=10'][1][0], shares['per=10'][1][1]))
    t.close()
    d_noisy.free(); d_genome.free()
    text = '\n'.join(out) + '\n'
    print('\n'.join(out[-2:]))
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
