"""
Object view of the scan C ABI (include/kvarq_hip.h) for callers that keep data
resident on the GPU: ``Table`` (the sequence list of ``engine.findseqs`` with
its seed index) and ``Scanner`` (``scan_filepart`` of the reference,
csrc/workhorse.c:976-1197, over batches that are already in device or host
memory).  ``engine.findseqs`` is the file-level entry; bench.py and the
multi-GPU driver use this module.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import view as _view
from .engine import Hit, _raise_last, scan_arrays, scan_hits, scan_records, scan_stats
from .options import ScanOptions


def _check(rc):
    if rc:
        _raise_last()


class Table(object):
    """target sequences (bytes or str) + engine config -> device table"""

    def __init__(self, seqs, **config):
        L = _lib.lib()
        self.seqs = [s.encode('latin-1') if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(self.seqs)
        cfg = _lib.Config()
        L.kvq_config_get(C.byref(cfg))
        for k, v in config.items():
            if k in ('Amin', 'Azero'):
                v = (v.encode('latin-1') if isinstance(v, str) else v)[0]
                v = v - 256 if v > 127 else v
            setattr(cfg, k, v)
        self.config = cfg
        bufs = [C.create_string_buffer(s, len(s) + 1) for s in self.seqs]
        arr = (C.c_char_p * max(1, n))(*[C.cast(b, C.c_char_p) for b in bufs])
        lens = (C.c_int32 * max(1, n))(*[len(s) for s in self.seqs])
        self.h = L.kvq_table_create(arr, lens, n, C.byref(cfg))
        if not self.h:
            _raise_last()
        self.nseq = n
        self.bases = L.kvq_table_bases(self.h)
        self.counters_len = L.kvq_counters_len(self.h)
        self.off_nseqhits = L.kvq_counters_off_nseqhits(self.h)
        self.off_nseqbasehits = L.kvq_counters_off_nseqbasehits(self.h)
        self.off_coverage = L.kvq_counters_off_coverage(self.h)
        self.off_mutations = L.kvq_counters_off_mutations(self.h)
        self.seq_offset = [L.kvq_table_seq_offset(self.h, i) for i in range(n + 1)]
        self.seeded = [bool(L.kvq_table_seq_is_seeded(self.h, i)) for i in range(n)]
        self.seed_k = L.kvq_table_seed_k(self.h)

    def close(self):
        if self.h:
            _lib.lib().kvq_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunk_offsets(data):
    """chunk cuts of fastq_read (workhorse.c:737-956) on an in-memory stream (numpy uint8 / bytes)"""
    L = _lib.lib()
    arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    cap = arr.nbytes // (512 * 1024) + 4
    out = (C.c_int64 * (cap + 1))()
    n = L.kvq_chunk_offsets(arr.ctypes.data if arr.nbytes else None, arr.nbytes, out, cap)
    if n < 0:
        raise RuntimeError('could find beginning of record')
    return np.array(list(out)[:n + 1], dtype=np.int64)


class RescanRequired(RuntimeError):
    """the hit arena overflowed on host batches that the Scanner no longer holds: reset() and feed them again"""


class Scanner(object):
    """accumulates hits and counters over any number of batches.

    Host batches (``scan_host``) cannot be replayed by the library when the hit arena turns out too small
    (``KVQ_ERR_RESCAN``); ``finish`` feeds them again itself from COPIES it keeps -- up to `retain_limit` bytes
    (the caller's buffers are never kept: they may be refilled).  Beyond that limit, or with ``retain_limit=0``,
    ``finish`` raises ``RescanRequired`` and the caller, who has the data, resets and feeds again; a caller with
    a re-readable source passes ``replay=callable`` (called with the scanner after ``reset()``) instead."""

    def __init__(self, table, counters_ptr=None, retain_limit=1 << 30, replay=None, **options):
        self.table = table
        # records, profile (True: the table's Amin), cycles, long_reads, per_read, duplication, overrepresented, adapters, clip, emit, emit_min, emit_compress (``options.ScanOptions``), set on the
        # scan handle once and kept across reset
        opt = ScanOptions(amin=bytes([table.config.Amin & 0xFF]), **options)
        self.records, self.profile, self.cycles, self.read_stats, self.long_reads = opt.records, opt.profile, opt.cycles, opt.read_stats, opt.long_reads
        self.overrepresented = opt.overrepresented
        self.adapters, self.adapter_names = opt.adapters, opt.adapter_names
        self.clip, self.clip_names = opt.clip, opt.clip_names      # (with ``clip`` the text of a batch is WRITTEN where it lies: ``scan_device``)
        # ``emit=True``: ``finish`` hands the emitted text back ('emitted'); ``emit=<path>``: it is streamed to that file, which is
        # created here and stays open until ``close``; ``emit_min``: the shortest read kept
        self.emit, self.emit_min, self._emit_file = opt.emit, opt.emit_min, None
        self.emit_compress = opt.emit_compress      # the emitted text leaves the GPU as BGZF: 'emitted' and the file hold that
        self.h = _lib.lib().kvq_scan_create(table.h, counters_ptr)
        if not self.h:
            _raise_last()
        for name, args in opt.setters():
            _check(getattr(_lib.lib(), name)(self.h, *args))
        if self.emit is not None and self.emit is not True:
            self._emit_file = open(self.emit, 'wb')
            _check(_lib.lib().kvq_scan_set_emit_fd(self.h, self._emit_file.fileno()))
        self._host_batches = []          # copies of what scan_host was given since the last reset (fed again when the hit arena overflows)
        self._device_batches = []        # what scan_device was given since the last reset (the caller's device memory: nothing is copied)
        self._retained, self._retain_limit, self._replay = 0, (0 if replay is not None else retain_limit), replay
        self._comm = None

    def set_comm(self, comm):
        """several GPUs (``dist.NativeComm``): ``finish`` becomes collective and sums the counters of all ranks over RCCL"""
        self._comm = comm
        _check(_lib.lib().kvq_scan_set_comm(self.h, comm.h if comm is not None else None))

    def gather_hits(self):
        """collective, after ``finish(hits=False)``: every rank's hits, in rank (= stream) order, on every rank;
        returns what ``finish`` returns for them"""
        _check(_lib.lib().kvq_scan_gather_hits(self.h, self._comm.h if self._comm is not None else None))
        return self._hits_dict()

    def force_exhaustive(self, on=True):
        _lib.lib().kvq_scan_force_exhaustive(self.h, 1 if on else 0)

    def scan_device(self, d_ptr, nbytes, chunk_off, fpos_base=0):
        """a batch in the caller's device memory.  With ``clip=`` THE BUFFER IS WRITTEN: the score bytes of every record from its
        adapter's first base on become '!' where they lie"""
        co = np.ascontiguousarray(chunk_off, dtype=np.int64)
        self._device_batches.append((d_ptr, nbytes, co, fpos_base))
        _check(_lib.lib().kvq_scan_device(self.h, d_ptr, nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1, fpos_base))

    def _feed_host(self, arr, co, fpos_base):
        _check(_lib.lib().kvq_scan_host(self.h, arr.ctypes.data if arr.nbytes else None, arr.nbytes,
                                        co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1, fpos_base))

    def scan_host(self, data, chunk_off=None, fpos_base=0):
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        co = chunk_offsets(arr) if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.int64)
        if self._host_batches is not None:
            if self._retained + arr.nbytes <= self._retain_limit:
                self._host_batches.append((arr.copy(), co.copy(), fpos_base)); self._retained += arr.nbytes
            else:
                self._host_batches = None          # too much to keep: an overflow is the caller's to replay
        self._feed_host(arr, co, fpos_base)

    def finish_begin(self):
        """every batch of this scan has been fed: enqueue the ordering of the hits and the copies to the host now
        (``kvq_scan_finish_begin``); ``finish`` then only waits.  For callers with several scanners in flight."""
        _check(_lib.lib().kvq_scan_finish_begin(self.h))

    def finish(self, hits=True, stats=True):
        """-> dict with 'hits', 'hitseqs' (bytes), 'stats', 'coverage', 'mutations', 'counters'.

        ``hits=False`` leaves hits and hit bytes in the library's arrays (``kvq_scan_hit_*``), ``stats=False``
        also skips the Python ``stats`` dict and hands out ``counters`` as a view of the library's host
        array (valid until the next ``reset`` / ``close``) -- for callers that only reduce counters."""
        L = _lib.lib()
        for attempt in range(4):
            if L.kvq_scan_finish(self.h) == 0:
                break
            if _lib.last_error()[0] != _lib.ERR_RESCAN or attempt == 3:
                _raise_last()
            # the hit arena was too small for the host batches (it has been enlarged): feed them again
            # (with a communicator the overflow may be another rank's: every rank goes round again, whatever it was fed with)
            again, device, replay = self._host_batches, self._device_batches, self._replay
            if again is None and replay is None:
                raise RescanRequired(_lib.last_error()[1])
            if replay is None and not again and not device:
                raise RescanRequired('nothing to feed again: ' + str(_lib.last_error()[1]))
            retained = self._retained
            self.reset()
            if replay is not None:
                replay(self)
            else:
                # the kept copies go in again as they are (no second copy, and they stay kept: a further round may want them);
                # device batches are the caller's memory and are simply named again
                self._host_batches, self._retained = again, retained
                for arr, co, fpos_base in again:
                    self._feed_host(arr, co, fpos_base)
                for d_ptr, nbytes, co, fpos_base in device:
                    self.scan_device(d_ptr, nbytes, co, fpos_base)
        t = self.table
        ctr = _view(L.kvq_scan_counters(self.h), t.counters_len, C.c_int64, np.int64)
        if stats:
            ctr = ctr.copy()
        out = {'counters': ctr}
        out['n_hits'] = L.kvq_scan_n_hits(self.h)
        if hits:
            out.update(self._hits_dict())
            if self.records:
                out['records'] = scan_records(L, self.h)      # the record of every hit (bytes), in the order of ``hits``
        if self.profile is not None:
            from . import profile as profile_
            out['profile'] = profile_.from_scan(L, self.h, adapters=(self.adapter_names, self.adapters))
            out['profile_kernel_ms'] = L.kvq_scan_profile_kernel_ms(self.h)
            if self.cycles:
                out['cycles_kernel_ms'] = L.kvq_scan_cycles_kernel_ms(self.h)
            if self.read_stats:
                out['reads_kernel_ms'] = L.kvq_scan_reads_kernel_ms(self.h)
            if self.overrepresented:
                out['over_kernel_ms'] = L.kvq_scan_over_kernel_ms(self.h)
            if self.adapters:
                out['adapt_kernel_ms'] = L.kvq_scan_adapt_kernel_ms(self.h)
        if self.clip:
            from . import profile as profile_
            out['clip'] = profile_.clip_from_scan(L, self.h, (self.clip_names, self.clip))
            out['clip_kernel_ms'] = L.kvq_scan_clip_kernel_ms(self.h)
        if self.emit is not None:
            from . import profile as profile_
            out['emit'] = profile_.emit_from_scan(L, self.h)
            out['emit_kernel_ms'] = L.kvq_scan_emit_kernel_ms(self.h)
            if self.emit_compress:
                out['emit_compress'] = profile_.emit_compress_from_scan(L, self.h)
                out['emit_deflate_kernel_ms'] = L.kvq_scan_emit_deflate_kernel_ms(self.h)
            if self.emit is True:
                out['emitted'] = profile_.emitted_from_scan(L, self.h)      # the emitted FastQ text, a numpy.uint8 array
        out['kernel_ms'] = L.kvq_scan_kernel_ms(self.h)
        out['main_kernel_ms'] = L.kvq_scan_main_kernel_ms(self.h)
        out['main_kernel_launches'] = L.kvq_scan_main_kernel_launches(self.h)
        if not stats:
            return out
        out['stats'] = scan_stats(L, self.h, t.nseq, 0, ctr)
        out['coverage'] = ctr[t.off_coverage:t.off_coverage + t.bases]
        out['mutations'] = ctr[t.off_mutations:t.off_mutations + 6 * t.bases]
        path = L.kvq_scan_path(self.h)
        out['path'] = {'seeded': bool(path & _lib.PATH_SEEDED), 'exhaustive': bool(path & _lib.PATH_EXHAUSTIVE),
                       'rescanned': bool(path & _lib.PATH_RESCANNED), 'tiles_rescanned': bool(path & _lib.PATH_TILES_RESCANNED)}
        if self.long_reads is not False:
            out['path']['read_list'] = bool(path & _lib.PATH_READ_LIST)      # a batch took the read-list route
        out['kernel'] = _lib.kernel_cell(L.kvq_scan_kernel(self.h))      # the scan kernel instantiation of the last seed-filter launch
        out['grid'] = L.kvq_scan_grid(self.h)                            # ... and its workgroups (0: no such launch)
        return out

    ORDER_INFO = ('n', 'nb', 'shift', 'bc', 'lo', 'crowded', 'mergesort', 'arena_cap', 'blob_cap')

    def order_info(self):
        """(measurement) ``kvq_scan_order_info``: how the finished scan's hits were put in order, and the capacities of
        the hit arena and the hit blob as they are now"""
        out = (C.c_int64 * 9)()
        _lib.lib().kvq_scan_order_info(self.h, out)
        return dict(zip(self.ORDER_INFO, (int(x) for x in out)))

    MATCH_INFO = ('survivors', 'survivors_cap', 'redo_records', 'redo_long')

    def match_info(self):
        """(measurement) ``kvq_scan_match_info``: the survivors' slots the finished scan's last seed-filter launch handed
        out, the slots its list has, the records its skipped tiles left to the redo and the long reads among them"""
        out = (C.c_int64 * 4)()
        _check(_lib.lib().kvq_scan_match_info(self.h, out))
        return dict(zip(self.MATCH_INFO, (int(x) for x in out)))

    LAUNCH_INFO = ('launches', 'pipelined', 'beside', 'sv_grid', 'sv_block', 'grid_cap', 'grid_cap_kind', 'cus', 'live_scans', 'last_beside')
    GRID_CAP_KINDS = (None, 'grid_full', 'grid_shared', 'KVQ_GRID')

    def launch_info(self):
        """(measurement) ``kvq_scan_launch_info``: the seed-filter launches of this scanner since it was made or reset -- how
        many, how many found the scan in front still running, how many published ahead of their survivors -- and of the
        last one the grid and block of kvq_verify_survivors, the grid cap and which it was, the CUs and the live scan
        objects.  All zero (``grid_cap_kind`` None) while there was no such launch.  Host-side facts: no device work"""
        out = (C.c_int64 * 10)()
        _lib.lib().kvq_scan_launch_info(self.h, out)
        d = dict(zip(self.LAUNCH_INFO, (int(x) for x in out)))
        d['grid_cap_kind'] = self.GRID_CAP_KINDS[d['grid_cap_kind']]
        d['last_beside'] = bool(d['last_beside'])
        return d

    def index_device(self, d_ptr, nbytes, chunk_off, cap=None):
        """(measurement) ``kvq_scan_index_device``: the exact record index of a batch in device memory -> (R, records per chunk,
        nl4 as an (n, 4) array, rec_start), n = min(R, cap); ``cap`` None: a quarter of the batch's bytes, which holds any index"""
        co = np.ascontiguousarray(chunk_off, dtype=np.int64)
        cap = nbytes // 4 + 1 if cap is None else cap
        nl4, rs, per = np.zeros((max(cap, 1), 4), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(len(co) - 1, 1), dtype=np.uint32)
        R = _lib.lib().kvq_scan_index_device(self.h, d_ptr, nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1,
                                             nl4.ctypes.data, rs.ctypes.data, cap, per.ctypes.data)
        if R < 0:
            _raise_last()
        n = min(R, cap)
        return R, per[:len(co) - 1], nl4[:n], rs[:n]

    def keep_skipped(self, on=True):
        """(measurement) ``kvq_scan_set_keep_skipped``: keep what ``skipped_tiles`` and ``redo_list`` report"""
        _check(_lib.lib().kvq_scan_set_keep_skipped(self.h, 1 if on else 0))

    SKIPPED_TILE = ('a', 'b', 'own_begin', 'own_end', 'seen', 'first')

    def skipped_tiles(self):
        """(measurement) ``kvq_scan_skipped_tiles``: the descriptors of the finished scan's skipped tiles, an (n, 6) array"""
        L = _lib.lib()
        n = L.kvq_scan_skipped_tiles(self.h, None, 0)
        if n < 0:
            _raise_last()
        out = np.zeros((max(n, 1), 6), dtype=np.uint32)
        L.kvq_scan_skipped_tiles(self.h, out.ctypes.data, n)
        return out[:n]

    def redo_list(self):
        """(measurement) ``kvq_scan_redo_list``: what kvq_collect_skipped left on the redo's list -> (nl4 (n, 4), rec_start)"""
        L = _lib.lib()
        n = L.kvq_scan_redo_list(self.h, None, None, 0)
        if n < 0:
            _raise_last()
        nl4, rs = np.zeros((max(n, 1), 4), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        L.kvq_scan_redo_list(self.h, nl4.ctypes.data, rs.ctypes.data, n)
        return nl4[:n], rs[:n]

    def hit_arrays(self):
        """the library's result arrays as numpy arrays (copies): seq_nr, file_pos, seq_pos, length, readlength,
        hitseq offsets (n + 1), hit bytes"""
        L = _lib.lib()
        out = {k: np.frombuffer(v, dtype=np.uint8) if k == 'blob' else v.copy() for k, v in scan_arrays(L, self.h).items()}
        nh = len(out['seq_nr'])
        if self.records:
            # hit i's record: record_blob[record_off[i] : record_off[i] + record_len[i]]
            out['record_off'] = _view(L.kvq_scan_hit_record_off(self.h), nh, C.c_int64, np.int64).copy()
            out['record_len'] = _view(L.kvq_scan_hit_record_len(self.h), nh, C.c_int32, np.int32).copy()
            nb = L.kvq_scan_record_bytes(self.h)
            out['record_blob'] = np.frombuffer(C.string_at(L.kvq_scan_record_blob(self.h), nb) if nb else b'', dtype=np.uint8)
        return out

    def _hits_dict(self):
        """the library's result arrays as the reference's ``hits`` tuple and ``hitseqs`` list (bytes)"""
        hits, hitseqs = scan_hits(_lib.lib(), self.h)
        return {'n_hits': len(hits), 'hits': hits, 'hitseqs': hitseqs}

    def reset(self):
        self._host_batches, self._device_batches, self._retained = [], [], 0
        _check(_lib.lib().kvq_scan_reset(self.h))

    def close(self):
        if self.h:
            _lib.lib().kvq_scan_destroy(self.h)
            self.h = None
        if getattr(self, '_emit_file', None) is not None:
            self._emit_file.close()
            self._emit_file = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer(object):
    """a plain device allocation (hipMalloc) with host copies in and out"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.ptr = _lib.lib().kvq_device_alloc(nbytes + 64)
        if not self.ptr:
            _raise_last()

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        _check(_lib.lib().kvq_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, nbytes=None, offset=0):
        n = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(n, dtype=np.uint8)
        _check(_lib.lib().kvq_memcpy_d2h(out.ctypes.data, self.ptr + offset, n))
        return out

    def free(self):
        if self.ptr:
            _lib.lib().kvq_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def inflate_bgzf_device(d_in, in_bytes, d_blocks, nblocks, d_out, out_bytes, d_status):
    """kvq_inflate_bgzf_device: inflate the BGZF members of a block table in device memory
    (kvq_bgzf_block entries: payload offset, output offset, payload bytes, isize) into d_out;
    d_status (device int32 per member) gets 0, -3 or -5 (zlib's codes).  Pointers are device
    addresses as ints (e.g. torch tensors' data_ptr()).  Blocks until done."""
    _check(_lib.lib().kvq_inflate_bgzf_device(C.c_void_p(d_in), in_bytes, C.c_void_p(d_blocks), nblocks,
                                               C.c_void_p(d_out), out_bytes, C.c_void_p(d_status)))


def deflate_bgzf_device(d_text, nbytes, d_out, out_cap):
    """kvq_deflate_bgzf_device: BGZF(d_text[0, nbytes)) -- the members, without the EOF member -- into
    d_out[0, out_cap), both device addresses as ints; ``kvq_deflate_bound(nbytes)`` bytes always hold it.  Returns (its length, the
    eight words); RuntimeError when out_cap is too small.  Blocks until done."""
    words = np.zeros(8, dtype=np.int64)
    n = _lib.lib().kvq_deflate_bgzf_device(C.c_void_p(d_text), nbytes, C.c_void_p(d_out), out_cap, words.ctypes.data_as(C.POINTER(C.c_int64)))
    if n < 0:
        _raise_last()
    return n, words


def inflate_gzip_device(d_file, n, chunk_bytes, d_out, out_cap):
    """kvq_inflate_gzip_device: a whole gzip file's bytes in device memory (d_file, n bytes) inflated
    by speculative chunk decoding into d_out (out_cap bytes; written only when the text fits).
    Returns (text length, report dict); kvarq_amd.gzip_spec.GzipError when the DEFLATE data fail,
    IOError for a missing gzip header.  Blocks until done."""
    from . import gzip_spec
    return gzip_spec._call(_lib.lib().kvq_inflate_gzip_device, C.c_void_p(d_file), n, chunk_bytes, out_cap, C.c_void_p(d_out))
