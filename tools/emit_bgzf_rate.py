#!/usr/bin/env python3
"""What the emit's deflate does (Scanner(emit=True, emit_compress=True)), written to profiles/emit_bgzf_rate.txt:
 (a) time: bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with the emit alone and with its deflate, alternately, medians of --reps steps each after two warm-ups: the step
     (scan to finish, wall), the GPU time of the batch's kernels, of the emit's kernels and of the deflate's, and the bytes that cross
     PCIe.  Whether the step gets shorter is the finding.
 (b) ratio: a --sample of the emitted text of that workload, and of tools/realistic_bench.py's text, through kvq_deflate_bgzf_device,
     beside zlib at level 1 and at level 6 on the same 65 280-byte blocks, on the host, as BGZF members (18 + 8 bytes around each
     raw stream).  The yardstick is zlib, not this code.
 (c) the host's way: the same sample through zlib at level 6 (bgzip's default) and level 1 on 16 threads, blocks dealt out in turn;
     the whole text's time is that of the sample times their ratio of bytes.
Nothing here is a condition: the numbers are reported.  The condition of the option -- off, the bench step is the parent's -- is
measured by bench.py on both trees, alternating, and written into the file by hand as (d), with the resource usage as (e), as in
profiles/emit_rate.txt.
"""
import argparse
import concurrent.futures
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from kvarq_amd import _lib, profile as P, scan, synth  # noqa: E402
from emit_rate import CFG, resident  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402
import realistic_bench  # noqa: E402

BLOCK = 65280
KEYS = ('kernel_ms', 'emit_kernel_ms', 'emit_deflate_kernel_ms')


def steps(L, scanners, d_data, nbytes, offs, reps):
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


def emitted_sample(t, d_data, reads, sample, rl=150):
    """the first ``sample`` bytes (whole blocks) of the emitted text of the resident batch: of as many of its first records as emit
    that much and half as much again (the whole emitted text is more than a Python bytes object is asked to hold at once)"""
    rb = synth.record_bytes(rl)
    n = min(reads, sample * 3 // 2 // rb + 1)
    nbytes, offs = n * rb, analytic_chunk_offsets(n, rb, rl)
    s = scan.Scanner(t, emit=True)
    s.scan_device(d_data.ptr, nbytes, offs)
    out = s.finish(hits=False, stats=False)['emitted']
    s.close()
    return out[:min(len(out), sample) // BLOCK * BLOCK].tobytes()


def zlib_blocks(text, level, threads=1):
    """(bytes of the BGZF members zlib makes of the text's blocks, seconds)"""
    def one(i):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(co.compress(text[i:i + BLOCK]) + co.flush()) + 26
    t0 = time.perf_counter()
    if threads == 1:
        n = sum(one(i) for i in range(0, len(text), BLOCK))
    else:
        with concurrent.futures.ThreadPoolExecutor(threads) as ex:
            n = sum(ex.map(one, range(0, len(text), BLOCK), chunksize=8))
    return n, time.perf_counter() - t0


def device_blocks(text):
    arr = np.frombuffer(text, dtype=np.uint8)
    cap = _lib.lib().kvq_deflate_bound(len(text))
    d_in, d_out = scan.DeviceBuffer(len(text)), scan.DeviceBuffer(cap)
    d_in.upload(arr)
    n, words = scan.deflate_bgzf_device(d_in.ptr, len(text), d_out.ptr, cap)
    d_in.free(); d_out.free()
    return n, P.deflate_words(words)


def ratio_lines(name, text):
    n, w = device_blocks(text)
    z1, t1 = zlib_blocks(text, 1)
    z6, t6 = zlib_blocks(text, 6)
    p1, tp1 = zlib_blocks(text, 1, 16)
    p6, tp6 = zlib_blocks(text, 6, 16)
    assert p1 == z1 and p6 == z6
    return ['    %-10s %11d bytes in %5d blocks: this code %10d (%.3f; %d stored, %.1f literals a match, longest match %d)   zlib -1 %10d (%.3f)   zlib -6 %10d (%.3f)'
            % (name, len(text), w['members'], n, len(text) / n, w['stored'], w['literals'] / max(w['matches'], 1), w['max_length'], z1, len(text) / z1, z6, len(text) / z6),
            '    %-10s this code makes %.1f %% more bytes than zlib -1 and %.1f %% more than zlib -6'
            % ('', 100.0 * (n - z1) / z1, 100.0 * (n - z6) / z6)], (t1, t6, tp1, tp6)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sample', type=int, default=64 << 20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'emit_bgzf_rate.txt'))
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    out = ['# tools/emit_bgzf_rate.py --reads %d --reps %d --sample %d' % (args.reads, args.reps, args.sample)]
    sc = {'emit': scan.Scanner(t, emit=True), 'emit_compress': scan.Scanner(t, emit=True, emit_compress=True)}
    for s in sc.values():
        s.emit = 'left in the library'                        # (finish then makes no numpy copy of the sink: gigabytes, and no part of the emit)
    med = steps(L, sc, d_data, nbytes, offs, args.reps)
    for s in sc.values():
        s.close()
    e, z = med['emit_compress'][1]['emit'], med['emit_compress'][1]['emit_compress']
    out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
               % (args.reads, nbytes / 1e9, args.reps))
    out.append('    %-14s step ms   batch kernels ms   emit kernels ms   deflate kernels ms   bytes over PCIe' % '')
    for k in sc:
        m = med[k][0]
        out.append('    %-14s %9.3f   %16.3f   %15.3f   %18.3f   %15d' % (k, m[0], m[1], m[2], m[3], e.bytes_out if k == 'emit' else z['bytes_out'] + 28))
    out.append('    ' + e.line())
    out.append('    emit bgzf: members=%d stored=%d bytes %d -> %d (%.3f); the deflate takes the text at %.2f GB/s'
               % (z['members'], z['stored'], z['bytes_in'], z['bytes_out'] + 28, z['ratio'], z['bytes_in'] / 1e6 / max(med['emit_compress'][0][3], 1e-9)))
    a, b = med['emit'][0], med['emit_compress'][0]
    out.append('    the step with the deflate is %.1f ms %s than with the emit alone: the deflate\'s kernels cost %.1f ms, the bytes that no longer cross save %.1f ms'
               % (abs(b[0] - a[0]), 'shorter' if b[0] < a[0] else 'LONGER', b[3], (a[1] - a[2]) - (b[1] - b[2] - b[3])))
    print('\n'.join(out)); sys.stdout.flush()
    bench_text = emitted_sample(t, d_data, args.reads, args.sample)
    d_data.free(); d_genome.free()
    rtext = realistic_bench.make_text(min(max(args.sample // 330, 1000), 100000), g)
    rarr = np.frombuffer(rtext, dtype=np.uint8) if not isinstance(rtext, np.ndarray) else rtext
    s = scan.Scanner(t, emit=True)
    s.scan_host(rarr)
    real_text = s.finish(hits=False, stats=False)['emitted']
    real_text = real_text[:len(real_text) // BLOCK * BLOCK].tobytes()
    s.close(); t.close()
    out.append('(b) ratio, on the first whole blocks of the emitted text (bytes in / bytes out; members with their 26 bytes, no EOF member)')
    host = {}
    for name, text in (('bench', bench_text), ('realistic', real_text)):
        lines, host[name] = ratio_lines(name, text)
        out += lines
    times, scale = host['bench'], e.bytes_out / float(len(bench_text))
    out.append('(c) the host\'s way, on the bench sample (%d bytes; the whole emitted text is %.1f times that): zlib -6 %.2f s on one thread, %.2f s on 16; zlib -1 %.2f s, %.2f s on 16'
               % (len(bench_text), scale, times[1], times[3], times[0], times[2]))
    out.append('    for the whole text that is %.1f s (zlib -6, 16 threads) and %.1f s (zlib -1, 16 threads) beside a step of %.3f s with the deflate on the device'
               % (times[3] * scale, times[2] * scale, b[0] / 1e3))
    text = '\n'.join(out) + '\n'
    print('\n'.join(out[len(out) - 7:]))
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
