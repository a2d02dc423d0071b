#!/usr/bin/env python3
"""End-to-end rate of engine.findseqs on plain gzip files: the host route (one zlib stream per file,
read by the serial reader) against the device route for any gzip (inflate='device_any': speculative
chunk decoding on the GPU).  A seeded FastQ of --reads x 150 bp (10 M: 3.25 GB)
is written as gzip at levels 1, 6 and 9 -- members of --member-mb of text each, compressed in
parallel, as pigz -i or a concatenation of gzip files would write them, or with --member-mb 0 one
single member, as gzip writes it --; per level the two routes
are timed alternately, --reps times each after one warm-up, page cache warm, in this one process.
Prints the medians, the device route's phase times and its report (engine.last_inflate_report()).
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kvarq_amd import _lib, engine, scan, synth  # noqa: E402

_DATA = None


def _open_text(path):
    global _DATA
    _DATA = np.memmap(path, dtype=np.uint8, mode='r')


def _member(args):
    lo, hi, level = args
    co = zlib.compressobj(level, zlib.DEFLATED, 31)                 # a whole gzip member
    out = [co.compress(_DATA[a:min(a + (64 << 20), hi)].tobytes()) for a in range(lo, hi, 64 << 20)]
    return b''.join(out) + co.flush()


def write_gzip(path, text_path, nbytes, level, procs, member):
    # the compressors are fresh processes ('spawn') that map the text from a file: they never inherit this process's GPU
    jobs = [(a, min(a + member, nbytes), level) for a in range(0, nbytes, member)]
    with mp.get_context('spawn').Pool(procs, initializer=_open_text, initargs=(text_path,)) as pool, open(path, 'wb') as f:
        for piece in pool.imap(_member, jobs):
            f.write(piece)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--levels', type=int, nargs='+', default=[1, 6, 9])
    ap.add_argument('--member-mb', type=int, default=256, help='text per gzip member; 0: the whole text in one member')
    ap.add_argument('--dir', default='/tmp')
    a = ap.parse_args()
    procs = min(16, len(os.sched_getaffinity(0)))
    L = 150
    rb = synth.record_bytes(L)
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')
    tag = '%dM' % (a.reads // 1_000_000) if a.reads >= 1_000_000 else '%dk' % (a.reads // 1000)
    mtag = 'one_member' if a.member_mb <= 0 else 'members_%dM' % a.member_mb
    paths = {lv: os.path.join(a.dir, 'kvq_gzip_rate_%s_%s_l%d.fastq.gz' % (tag, mtag, lv)) for lv in a.levels}
    need = [lv for lv in a.levels if not os.path.exists(paths[lv])]
    if need:
        dg = scan.DeviceBuffer(g.nbytes); dg.upload(g)
        dd = scan.DeviceBuffer(a.reads * rb)
        _lib.lib().kvq_synth_reads_device(dd.ptr, 0, a.reads, L, synth.SEED, dg.ptr, g.nbytes)
        data = dd.download()
        dd.free(); dg.free()
        text_path = os.path.join(a.dir, 'kvq_gzip_rate_%s.fastq' % tag)
        data.tofile(text_path)
        del data
        for lv in need:
            t0 = time.perf_counter()
            write_gzip(paths[lv], text_path, a.reads * rb, lv, procs, a.member_mb << 20 if a.member_mb > 0 else a.reads * rb)
            print('wrote %s (%.2f GB) in %.1f s' % (paths[lv], os.path.getsize(paths[lv]) / 1e9, time.perf_counter() - t0), flush=True)
        os.remove(text_path)
    text = a.reads * rb
    for lv in a.levels:
        comp = os.path.getsize(paths[lv])
        times = {'host': [], 'device_any': []}
        ref, rep = None, None
        for it in range(a.reps + 1):                                   # it 0: warm-up (page cache, pinned buffers, kept scan)
            for route in ('host', 'device_any'):
                engine.config(**dict(cfg, nthreads=16))
                t0 = time.perf_counter()
                r = engine.findseqs(paths[lv], seqs, inflate=route)
                dt = time.perf_counter() - t0
                want = 'host' if route == 'host' else 'device_gzip'
                assert engine.last_inflate() == want, (route, engine.last_inflate())
                key = (len(r['hits']), r['stats']['parsed'], r['stats']['total'], r['stats']['records_parsed'])
                ref = ref or key
                assert key == ref, (route, key, ref)
                if it:
                    times[route].append(dt)
                if route != 'host':
                    rep = engine.last_inflate_report()
        for route in ('host', 'device_any'):
            best, med = min(times[route]), sorted(times[route])[len(times[route]) // 2]
            row = dict(level=lv, route=route, members=mtag, nthreads=16, reads=a.reads, text_bytes=text, compressed_bytes=comp, seconds=times[route],
                       median_s=med, reads_per_s=a.reads / med, inflated_GB_per_s=text / med / 1e9, hits=ref[0])
            if route != 'host':
                row['report'] = rep
            print('level %d  %-10s  median %.3f s (best %.3f)  %.1f M reads/s  %.2f GB/s inflated  hits=%d'
                  % (lv, route, med, best, a.reads / med / 1e6, text / med / 1e9, ref[0]), flush=True)
            if route != 'host':
                print('    phases (last call): find %.1f  decode %.1f  resolve %.1f  replace %.1f ms; runs %d chunks %d refuted %d '
                      'redecodes %d overflows %d markers %d candidates tested %d'
                      % (rep['ms_find'], rep['ms_decode'], rep['ms_resolve'], rep['ms_replace'], rep['runs'], rep['chunks'], rep['refuted'],
                         rep['redecodes'], rep['slot_overflows'], rep['marker_symbols'], rep['candidates_tested']), flush=True)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
