#!/usr/bin/env python3
"""End-to-end rate of engine.findseqs on BGZF (bgzip) files: the host route (block-parallel
inflate on the CPU, nthreads=16) against the device route (inflate='device': the blocks are
inflated, cut and scanned on the GPU).  A seeded FastQ of --reads x 150 bp (10 M: 3.25 GB) is
written as BGZF (bgzip's 65 280-byte blocks) at levels 1 and 6; per level the two routes are
timed alternately, --reps times each, in this one process.

--profile: one device-route call on the level-6 file (written before by a full run, or now),
for a run under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import multiprocessing as mp
import os
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kvarq_amd import _lib, engine, scan, synth  # noqa: E402

BLOCK = 65280                      # bgzip's block: 0xff00 bytes of text
EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
_DATA = None


def _open_text(path):
    global _DATA
    _DATA = np.memmap(path, dtype=np.uint8, mode='r')


def _blocks(args):
    lo, hi, level = args
    out = []
    for a in range(lo, hi, BLOCK):
        chunk = _DATA[a:min(a + BLOCK, hi)].tobytes()
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = co.compress(chunk) + co.flush()
        out.append(b'\x1f\x8b\x08\x04\0\0\0\0\x00\xff' + struct.pack('<H', 6) + b'BC' + struct.pack('<HH', 2, len(raw) + 25) +
                   raw + struct.pack('<II', zlib.crc32(chunk), len(chunk)))
    return b''.join(out)


def write_bgzf(path, text_path, nbytes, level, procs):
    # the compressors are fresh processes ('spawn') that map the text from a file: they never inherit this process's GPU
    step = BLOCK * 256
    jobs = [(a, min(a + step, nbytes), level) for a in range(0, nbytes, step)]
    with mp.get_context('spawn').Pool(procs, initializer=_open_text, initargs=(text_path,)) as pool, open(path, 'wb') as f:
        for piece in pool.imap(_blocks, jobs):
            f.write(piece)
        f.write(EOF_BLOCK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--levels', type=int, nargs='+', default=[1, 6])
    ap.add_argument('--dir', default='/tmp')
    ap.add_argument('--profile', action='store_true')
    a = ap.parse_args()
    procs = min(16, len(os.sched_getaffinity(0)))
    L = 150
    rb = synth.record_bytes(L)
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')
    paths = {lv: os.path.join(a.dir, 'kvq_bgzf_rate_%dM_l%d.fastq.gz' % (a.reads // 1_000_000, lv)) for lv in a.levels}
    need = [lv for lv in a.levels if not os.path.exists(paths[lv])]
    if need:
        dg = scan.DeviceBuffer(g.nbytes); dg.upload(g)
        dd = scan.DeviceBuffer(a.reads * rb)
        _lib.lib().kvq_synth_reads_device(dd.ptr, 0, a.reads, L, synth.SEED, dg.ptr, g.nbytes)
        data = dd.download()
        dd.free(); dg.free()
        text_path = os.path.join(a.dir, 'kvq_bgzf_rate_%dM.fastq' % (a.reads // 1_000_000))
        data.tofile(text_path)
        del data
        for lv in need:
            t0 = time.perf_counter()
            write_bgzf(paths[lv], text_path, a.reads * rb, lv, procs)
            print('wrote %s (%.2f GB) in %.1f s' % (paths[lv], os.path.getsize(paths[lv]) / 1e9, time.perf_counter() - t0), flush=True)
        os.remove(text_path)
    text = a.reads * rb
    if a.profile:
        engine.config(**dict(cfg, nthreads=16))
        for lv in a.levels:
            t0 = time.perf_counter()
            r = engine.findseqs(paths[lv], seqs, inflate='device')
            assert engine.last_inflate() == 'device'
            dt = time.perf_counter() - t0
            print('profile level %d: %.3f s  %.1f M reads/s  hits=%d' % (lv, dt, a.reads / dt / 1e6, len(r['hits'])), flush=True)
        return
    for lv in a.levels:
        comp = os.path.getsize(paths[lv])
        times = {'host': [], 'device': []}
        ref = None
        for rep in range(a.reps + 1):                                  # rep 0: warm-up (page cache, pinned buffers, kept scan)
            for route in ('host', 'device'):
                engine.config(**dict(cfg, nthreads=16))
                t0 = time.perf_counter()
                r = engine.findseqs(paths[lv], seqs, inflate=route)
                dt = time.perf_counter() - t0
                assert engine.last_inflate() == route, (route, engine.last_inflate())
                key = (len(r['hits']), r['stats']['parsed'], r['stats']['total'], r['stats']['records_parsed'])
                ref = ref or key
                assert key == ref, (route, key, ref)
                if rep:
                    times[route].append(dt)
        for route in ('host', 'device'):
            best, med = min(times[route]), sorted(times[route])[len(times[route]) // 2]
            row = dict(level=lv, route=route, nthreads=16, reads=a.reads, text_bytes=text, compressed_bytes=comp, seconds=times[route],
                       median_s=med, reads_per_s=a.reads / med, inflated_GB_per_s=text / med / 1e9, hits=ref[0])
            print('level %d  %-6s  median %.3f s (best %.3f)  %.1f M reads/s  %.2f GB/s inflated  hits=%d'
                  % (lv, route, med, best, a.reads / med / 1e6, text / med / 1e9, ref[0]), flush=True)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
