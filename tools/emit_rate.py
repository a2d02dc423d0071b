#!/usr/bin/env python3
"""What the emit costs (Scanner(emit=True)), written to profiles/emit_rate.txt:
 (a) bench.py's workload -- --reads x 150 bp resident in HBM, the MTBC-shaped table, the product config -- through
     scan.Scanner with nothing and with the emit, alternately, --reps steps each after two warm-ups: the step (scan to finish,
     wall), the GPU time of the batch's kernels, the scan kernel alone, and the emit's kernels alone (kvq_emit_size, the prefix sum,
     kvq_emit_copy: kvq_scan_emit_kernel_ms).  The batch's span of events closes behind the emit, so it holds the host's wait too:
     what the span grows by with the emit on, less the emit's kernels, is the emitted bytes on their way through the two pinned
     halves and their append to the sink.
 (b) beside it, in the same session: a device-to-device copy of as many bytes as were emitted (the copy the hardware allows), and
     their copy to pinned host memory (the way out the hardware allows): hipMemcpyAsync, timed with HIP events.
Nothing here is a condition: the numbers are reported.  The condition of the option -- off, the bench step is the parent's -- is
measured by bench.py on both trees and written into the file by hand, as in profiles/clip_rate.txt.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvarq_amd import _lib, scan, synth  # noqa: E402
from bench import analytic_chunk_offsets  # noqa: E402

CFG = dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.')      # kvarq/config.py:2-10
KEYS = ('kernel_ms', 'main_kernel_ms', 'emit_kernel_ms')


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
            r.pop('emitted', None)                        # (gigabytes: not kept from step to step)
            last[k] = r
            if rep >= 2:
                res[k].append([(t1 - t0) * 1e3] + [r.get(key, 0.0) for key in KEYS])
    return {k: ([statistics.median(x[i] for x in v) for i in range(1 + len(KEYS))], last[k]) for k, v in res.items()}


def plain_copies(nbytes, reps):
    """(ms of a device-to-device hipMemcpyAsync of nbytes, ms of their hipMemcpyAsync to pinned host memory), medians; the HIP
    runtime the library runs on, called directly"""
    import ctypes as C
    hip = C.CDLL('libamdhip64.so')
    D2H, D2D = 2, 3                                           # hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice

    def ok(rc):
        if rc:
            raise SystemExit('HIP error %d' % rc)
    src, dst = scan.DeviceBuffer(nbytes), scan.DeviceBuffer(nbytes)
    ok(_lib.lib().kvq_memset_d(src.ptr, 65, nbytes))
    pin = C.c_void_p()
    ok(hip.hipHostMalloc(C.byref(pin), C.c_size_t(nbytes), C.c_uint(0)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))
    out = []
    for to, kind in ((C.c_void_p(dst.ptr), D2D), (pin, D2H)):
        ms = []
        for rep in range(reps + 2):
            ok(hip.hipEventRecord(ev[0], None))
            ok(hip.hipMemcpyAsync(to, C.c_void_p(src.ptr), C.c_size_t(nbytes), C.c_int(kind), None))
            ok(hip.hipEventRecord(ev[1], None))
            ok(hip.hipEventSynchronize(ev[1]))
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]))
            if rep >= 2:
                ms.append(t.value)
        out.append(statistics.median(ms))
    for e in ev:
        hip.hipEventDestroy(e)
    hip.hipHostFree(pin)
    src.free(); dst.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'emit_rate.txt'))
    args = ap.parse_args()
    L = _lib.lib()
    g, d_genome, d_data, offs, nbytes = resident(L, args.reads)
    t = scan.Table(synth.both_strands(synth.table(g, 'MTBC')), **CFG)
    out = ['# tools/emit_rate.py --reads %d --reps %d' % (args.reads, args.reps)]
    sc = {'off': scan.Scanner(t), 'emit': scan.Scanner(t, emit=True)}
    sc['emit'].emit = 'left in the library'                   # (finish then makes no numpy copy of the sink: gigabytes, and no part of the emit)
    med = steps(L, sc, d_data, nbytes, offs, args.reps)
    for s in sc.values():
        s.close()
    e = med['emit'][1]['emit']
    out.append('(a) %d reads x 150 bp resident (%.2f GB), MTBC table, product config; Scanner, one batch; medians of %d steps each, alternating'
               % (args.reads, nbytes / 1e9, args.reps))
    out.append('    %-8s step ms   batch kernels ms   scan kernel ms   emit kernels ms (GB/s of text + emitted)' % '')
    for k in sc:
        m = med[k][0]
        rate = '(%.0f)' % ((nbytes + e.bytes_out) / 1e6 / m[3]) if m[3] else ''
        out.append('    %-8s %9.3f   %16.3f   %14.3f   %15.3f %s' % (k, m[0], m[1], m[2], m[3], rate))
    out.append('    ' + e.line())
    print('\n'.join(out)); sys.stdout.flush()
    d_data.free(); d_genome.free(); t.close()
    L.kvq_release_cached()
    d2d, d2h = plain_copies(e.bytes_out, args.reps)
    out.append('(b) the same %d bytes in the same session: device to device %.3f ms (%.0f GB/s read + written), device to pinned host %.3f ms (%.1f GB/s)'
               % (e.bytes_out, d2d, 2 * e.bytes_out / 1e6 / d2d, d2h, e.bytes_out / 1e6 / d2h))
    m, off = med['emit'][0], med['off'][0]
    wait = m[1] - off[1] - m[3]
    out.append('    the emit\'s kernels take %.2fx the plain device copy of their output; of the step\'s %.1f ms with the emit on, %.1f ms (%.0f %%) are the host\'s wait: the bytes'
               % (m[3] / d2d, m[0], wait, 100 * wait / m[0]))
    out.append('    through the pinned halves and their append to the sink (the plain copy to pinned memory alone: %.1f ms)' % d2h)
    text = '\n'.join(out) + '\n'
    print('\n'.join(out[-3:]))
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
