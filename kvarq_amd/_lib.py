"""ctypes binding of libkvarq_hip.so (include/kvarq_hip.h).  There is no CPU
fallback: if the library is missing, import fails loudly; if no GPU is present,
every compute entry point reports KVQ_ERR_DEVICE."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'libkvarq_hip.so')

MAX_READLENGTH = 1024
OK, ERR_FORMAT, ERR_IO, ERR_MEMORY, ERR_RUNTIME, ERR_TYPE, ERR_DEVICE, ERR_RESCAN = range(8)
CTR_RECORDS, CTR_LONGEST, CTR_HITS, CTR_READLENGTHS = 0, 1, 2, 4
CELL_DENSE, CELL_DIAG, CELL_STAMPS = 0x1000, 0x2000, 0x4000      # kvq_scan_kernel_pick / kvq_scan_kernel
FIND_RECORDS = 4                                                 # kvq_findseqs_ex: keep the records of the hits
FIND_PROFILE = 8                                                 # kvq_findseqs_opts: profile the input
FIND_CYCLES = 16                                                 # ... and count its bytes per cycle (with FIND_PROFILE)
FIND_READ_STATS, FIND_DUPLICATION = 128, 256                     # ... the per-read distributions, the duplication (with FIND_PROFILE)
FIND_OVERREPRESENTED = 512                                       # ... the overrepresented sequences (with FIND_PROFILE)
FIND_ADAPTERS = 1024                                             # ... the adapter content (with FIND_PROFILE; the probes in FindOptsAdapters)
FIND_CLIP = 2048                                                 # ... the adapter clip ahead of the trim (no profile needed; the same probe block)
FIND_ADAPTER_MISMATCHES = 4096                                   # ... the probes of both tolerate mismatches (the rate in FindOptsAdaptersMm)
FIND_EMIT = 8192                                                 # ... the trimmed reads as FastQ text (min_length and the output's path in FindOptsEmit)
FIND_EMIT_BGZF = 16384                                           # ... deflated to BGZF on the device (read only with FIND_EMIT)
READ_STATS, READ_DUPLICATION = 1, 2                           # kvq_scan_set_read_stats
FIND_LONG_READS, FIND_LONG_READS_AUTO = 32, 64                   # kvq_findseqs_ex / _opts: the read-list route, always / by the batch's head
LONG_READS_MODES = {False: 0, True: 1, 'auto': 2}                # kvq_scan_set_long_reads
# kvq_scan_path: a batch took the seed-filter kernel / the exhaustive kernels; a whole batch / the records of skipped tiles were redone;
# the text was inflated on the device (bit 4; bit 5: a file by speculative gzip decoding; bit 6: BAM records); a batch took the read-list route
PATH_SEEDED, PATH_EXHAUSTIVE, PATH_RESCANNED, PATH_TILES_RESCANNED = 1, 2, 4, 8
PATH_DEVICE_INFLATE, PATH_DEVICE_GZIP, PATH_DEVICE_BAM, PATH_READ_LIST = 0x10, 0x20, 0x40, 0x80


def long_reads_mode(long_reads):
    """the mode of kvq_scan_set_long_reads for a ``long_reads`` option (False, True or 'auto')"""
    if not isinstance(long_reads, (bool, str)) or long_reads not in LONG_READS_MODES:
        raise ValueError("long_reads must be False, True or 'auto'")
    return LONG_READS_MODES[long_reads]


class Config(C.Structure):
    _fields_ = [('maxerrors', C.c_int32), ('minoverlap', C.c_int32), ('minreadlength', C.c_int32),
                ('nthreads', C.c_int32), ('Amin', C.c_int8), ('Azero', C.c_int8)]


class LiveStats(C.Structure):
    _fields_ = [('records_parsed', C.c_int64), ('parsed', C.c_int64), ('total', C.c_int64),
                ('rls_longest', C.c_int64), ('nseq', C.c_int32), ('running', C.c_int32),
                ('sigints', C.c_int32), ('stop_requested', C.c_int32)]


class FindOpts(C.Structure):
    _fields_ = [('size', C.c_uint32), ('flags', C.c_uint32), ('n_cutoffs', C.c_int32), ('cutoffs', C.c_uint8 * 8)]


class FindOptsAdapters(C.Structure):
    """kvq_find_opts_adapters: the 20 bytes of kvq_find_opts, then the probes of FIND_ADAPTERS"""
    _fields_ = [('base', FindOpts), ('n_probes', C.c_int32), ('lens', C.c_uint8 * 8), ('probes', (C.c_uint8 * 32) * 8)]


class FindOptsAdaptersMm(C.Structure):
    """kvq_find_opts_adapters_mm: kvq_find_opts_adapters, then the mismatch rate of FIND_ADAPTER_MISMATCHES"""
    _fields_ = [('a', FindOptsAdapters), ('mismatch_per', C.c_int32)]


class FindOptsEmit(C.Structure):
    """kvq_find_opts_emit: kvq_find_opts_adapters_mm, then min_length and the output's path of FIND_EMIT"""
    _fields_ = [('m', FindOptsAdaptersMm), ('min_length', C.c_int32), ('path', C.c_char_p)]


class GzipReport(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('runs', 'chunks', 'candidates_tested', 'refuted', 'redecodes',
                                         'slot_overflows', 'marker_symbols', 'input_retries')] + \
        [(n, C.c_double) for n in ('ms_find', 'ms_decode', 'ms_resolve', 'ms_replace')]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BamReport(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('runs', 'segments', 'refuted', 'check_passes', 'records_seen', 'records_written',
                                         'records_skipped', 'records_noqual', 'bam_bytes', 'text_bytes')] + \
        [(n, C.c_double) for n in ('ms_inflate', 'ms_find', 'ms_emit')]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


i32, i64, u64, vp, cp = C.c_int32, C.c_int64, C.c_uint64, C.c_void_p, C.c_char_p
P = C.POINTER

# name -> (restype, argtypes): every symbol include/kvarq_hip.h declares
PROTOTYPES = {
    'kvq_config_set': (None, [P(Config)]),
    'kvq_config_get': (None, [P(Config)]),
    'kvq_last_error': (i32, [C.c_char_p, C.c_size_t]),
    'kvq_table_create': (vp, [P(cp), P(i32), i32, P(Config)]),
    'kvq_table_destroy': (None, [vp]),
    'kvq_table_nseq': (i32, [vp]),
    'kvq_table_bases': (i64, [vp]),
    'kvq_table_seq_is_seeded': (i32, [vp, i32]),
    'kvq_table_seed_k': (i32, [vp]),
    'kvq_counters_len': (i64, [vp]),
    'kvq_counters_off_nseqhits': (i64, [vp]),
    'kvq_counters_off_nseqbasehits': (i64, [vp]),
    'kvq_counters_off_coverage': (i64, [vp]),
    'kvq_counters_off_mutations': (i64, [vp]),
    'kvq_table_seq_offset': (i64, [vp, i32]),
    'kvq_scan_create': (vp, [vp, vp]),
    'kvq_scan_destroy': (None, [vp]),
    'kvq_chunk_offsets': (i64, [vp, i64, P(i64), i64]),
    'kvq_scan_device': (i32, [vp, vp, i64, P(i64), i64, i64]),
    'kvq_scan_host': (i32, [vp, vp, i64, P(i64), i64, i64]),
    'kvq_scan_host_async': (i32, [vp, vp, i64, P(i64), i64, i64]),
    'kvq_scan_host_copied': (i32, [vp]),
    'kvq_scan_host_drain': (i32, [vp]),
    'kvq_scan_finish': (i32, [vp]),
    'kvq_scan_finish_begin': (i32, [vp]),
    'kvq_scan_n_hits': (i64, [vp]),
    'kvq_scan_hit_seq_nr': (P(i32), [vp]),
    'kvq_scan_hit_file_pos': (P(i64), [vp]),
    'kvq_scan_hit_seq_pos': (P(i32), [vp]),
    'kvq_scan_hit_length': (P(i32), [vp]),
    'kvq_scan_hit_readlength': (P(i32), [vp]),
    'kvq_scan_hitseq_blob': (vp, [vp]),
    'kvq_scan_hitseq_offsets': (P(i64), [vp]),
    'kvq_scan_counters': (P(i64), [vp]),
    'kvq_scan_device_counters': (vp, [vp]),
    'kvq_scan_device_counters_own': (vp, [vp]),
    'kvq_scan_parsed': (i64, [vp]),
    'kvq_scan_total': (i64, [vp]),
    'kvq_scan_set_records': (i32, [vp, i32]),
    'kvq_scan_set_long_reads': (i32, [vp, i32]),
    'kvq_scan_record_blob': (vp, [vp]),
    'kvq_scan_hit_record_off': (P(i64), [vp]),
    'kvq_scan_hit_record_len': (P(i32), [vp]),
    'kvq_scan_record_bytes': (i64, [vp]),
    'kvq_profile_len': (i64, [i32]),
    'kvq_scan_set_profile': (i32, [vp, vp, i32]),
    'kvq_scan_profile': (P(i64), [vp]),
    'kvq_scan_profile_cutoffs': (i32, [vp, vp]),
    'kvq_profile_host': (i32, [vp, i64, P(i64), i64, vp, i32, P(i64)]),
    'kvq_cycles_len': (i64, []),
    'kvq_scan_set_cycles': (i32, [vp, i32]),
    'kvq_scan_cycles': (P(i64), [vp]),
    'kvq_cycles_host': (i32, [vp, i64, P(i64), i64, P(i64)]),
    'kvq_reads_len': (i64, []),
    'kvq_dup_len': (i64, []),
    'kvq_scan_set_read_stats': (i32, [vp, i32]),
    'kvq_scan_reads': (P(i64), [vp]),
    'kvq_scan_dup': (P(i64), [vp]),
    'kvq_reads_host': (i32, [vp, i64, P(i64), i64, i64, P(i64), P(i64)]),
    'kvq_dup_hash_host': (u64, [vp, i64]),
    'kvq_scan_reads_kernel_ms': (C.c_double, [vp]),
    'kvq_over_len': (i64, []),
    'kvq_scan_set_overrepresented': (i32, [vp, i32]),
    'kvq_scan_over': (P(i64), [vp]),
    'kvq_over_host': (i32, [vp, i64, P(i64), i64, i64, P(i64)]),
    'kvq_scan_over_kernel_ms': (C.c_double, [vp]),
    'kvq_adapt_len': (i64, []),
    'kvq_scan_set_adapters': (i32, [vp, P(cp), P(i32), i32]),
    'kvq_scan_adapters': (P(i64), [vp]),
    'kvq_adapt_host': (i32, [vp, i64, P(i64), i64, P(cp), P(i32), i32, P(i64)]),
    'kvq_scan_adapt_kernel_ms': (C.c_double, [vp]),
    'kvq_clip_len': (i64, []),
    'kvq_scan_set_clip': (i32, [vp, P(cp), P(i32), i32]),
    'kvq_scan_clip': (P(i64), [vp]),
    'kvq_clip_host': (i32, [vp, i64, P(i64), i64, P(cp), P(i32), i32, P(i64)]),
    'kvq_scan_clip_kernel_ms': (C.c_double, [vp]),
    'kvq_scan_set_adapter_mismatches': (i32, [vp, i32]),
    'kvq_scan_adapter_mismatches': (i32, [vp]),
    'kvq_adapt_host_mm': (i32, [vp, i64, P(i64), i64, P(cp), P(i32), i32, i32, P(i64)]),
    'kvq_clip_host_mm': (i32, [vp, i64, P(i64), i64, P(cp), P(i32), i32, i32, P(i64)]),
    'kvq_emit_len': (i64, []),
    'kvq_scan_set_emit': (i32, [vp, i32, i32]),
    'kvq_scan_set_emit_fd': (i32, [vp, i32]),
    'kvq_scan_emitted': (i32, [vp, P(vp), P(i64)]),
    'kvq_scan_emit': (P(i64), [vp]),
    'kvq_scan_emit_guard': (i64, [vp]),
    'kvq_scan_emit_kernel_ms': (C.c_double, [vp]),
    'kvq_emit_host': (i64, [vp, i64, P(i64), i64, i32, i32, vp, i64, P(i64)]),
    'kvq_deflate_len': (i64, []),
    'kvq_deflate_bound': (i64, [i64]),
    'kvq_bgzf_eof': (vp, []),
    'kvq_scan_set_emit_compress': (i32, [vp, i32]),
    'kvq_scan_emit_compress': (P(i64), [vp]),
    'kvq_scan_emit_deflate_kernel_ms': (C.c_double, [vp]),
    'kvq_deflate_bgzf_device': (i64, [vp, i64, vp, i64, P(i64)]),
    'kvq_deflate_bgzf_host': (i64, [vp, i64, vp, i64, P(i64)]),
    'kvq_deflate_lengths_host': (i32, [vp, i32, i32, vp]),
    'kvq_scan_kernel_ms': (C.c_double, [vp]),
    'kvq_scan_main_kernel_ms': (C.c_double, [vp]),
    'kvq_scan_profile_kernel_ms': (C.c_double, [vp]),
    'kvq_scan_cycles_kernel_ms': (C.c_double, [vp]),
    'kvq_scan_gap_ms': (C.c_double, [vp, vp]),
    'kvq_scan_order_info': (None, [vp, P(i64)]),
    'kvq_scan_match_info': (i32, [vp, P(i64)]),
    'kvq_scan_launch_info': (None, [vp, P(i64)]),
    'kvq_scan_index_device': (i64, [vp, vp, i64, P(i64), i64, vp, vp, i64, vp]),
    'kvq_scan_set_keep_skipped': (i32, [vp, i32]),
    'kvq_scan_skipped_tiles': (i64, [vp, vp, i64]),
    'kvq_scan_redo_list': (i64, [vp, vp, vp, i64]),
    'kvq_scan_main_kernel_launches': (i64, [vp]),
    'kvq_scan_reset': (i32, [vp]),
    'kvq_scan_path': (i32, [vp]),
    'kvq_scan_force_exhaustive': (None, [vp, i32]),
    'kvq_scan_kernel_pick': (i32, [i32, i32, i32, C.c_uint32, C.c_uint32, C.c_uint32]),
    'kvq_scan_kernel': (i32, [vp]),
    'kvq_scan_grid': (i32, [vp]),
    'kvq_tile_for_text': (C.c_uint32, [vp, C.c_size_t, P(C.c_uint32)]),
    'kvq_comm_unique_id': (i32, [vp]),
    'kvq_comm_create': (vp, [i32, i32, vp]),
    'kvq_comm_destroy': (None, [vp]),
    'kvq_comm_nranks': (i32, [vp]),
    'kvq_comm_rank': (i32, [vp]),
    'kvq_scan_set_comm': (i32, [vp, vp]),
    'kvq_scan_gather_hits': (i32, [vp, vp]),
    'kvq_comm_allreduce_counters': (i32, [vp, vp, i64, vp]),
    'kvq_comm_create_local': (vp, [i32, i32, C.c_uint64]),
    'kvq_gather_plan': (i32, [i32, vp, vp, vp, vp]),
    'kvq_gather_host': (i32, [i32, vp, vp, vp]),
    'kvq_result_layout_words': (None, [C.c_uint64, C.c_uint64, vp]),
    'kvq_findseqs': (vp, [P(cp), i32, P(cp), P(i32), i32]),
    'kvq_findseqs_ex': (vp, [P(cp), i32, P(cp), P(i32), i32, C.c_uint32]),
    'kvq_findseqs_opts': (vp, [P(cp), i32, P(cp), P(i32), i32, P(FindOpts)]),
    'kvq_findseqs_free': (None, [vp]),
    'kvq_host_chunk_plan': (i64, [P(cp), i32, P(i64), P(i64), i64, P(i64), P(i64), i64]),
    'kvq_poll_stats': (None, [P(LiveStats), P(i64), P(i64), P(i64), i32]),
    'kvq_request_stop': (None, []),
    'kvq_count_sigint': (None, []),
    'kvq_sigint_counter_install': (C.c_int, []),
    'kvq_sigint_counter_remove': (None, []),
    'kvq_device_count': (i32, []),
    'kvq_set_device': (i32, [i32]),
    'kvq_device_alloc': (vp, [i64]),
    'kvq_device_free': (None, [vp]),
    'kvq_memcpy_h2d': (i32, [vp, vp, i64]),
    'kvq_memcpy_d2h': (i32, [vp, vp, i64]),
    'kvq_memset_d': (i32, [vp, i32, i64]),
    'kvq_device_synchronize': (i32, []),
    'kvq_release_cached': (None, []),
    'kvq_synth_reads_device': (i32, [vp, i64, i64, i32, u64, vp, i64]),
    'kvq_synth_reads_host': (None, [vp, i64, i64, i32, u64, vp, i64]),
    'kvq_synth_genome_host': (None, [vp, i64, u64]),
    'kvq_inflate_raw_host': (i32, [vp, i64, vp, i64]),
    'kvq_bgzf_index': (i64, [vp, i64, P(i64), P(C.c_uint32), P(C.c_uint32), i64]),
    'kvq_chunk_offsets_device': (i64, [vp, i64, P(i64), i64]),
    'kvq_inflate_bgzf_device': (i32, [vp, i64, vp, i64, vp, i64, vp]),
    'kvq_inflate_gzip_host': (i64, [vp, i64, i64, vp, i64, P(i32), P(i64), P(GzipReport)]),
    'kvq_inflate_gzip_device': (i64, [vp, i64, i64, vp, i64, P(i32), P(i64), P(GzipReport)]),
    'kvq_gzip_last_report': (None, [P(GzipReport)]),
    'kvq_gzip_slot_canaries': (i64, [i32]),
    'kvq_gzip_last_chunks': (i64, [P(i64), i64, P(i64), P(i64), P(i64), i64, P(i64)]),
    'kvq_bam_last_report': (None, [P(BamReport)]),
    'kvq_bam_header_host': (i64, [vp, i64, P(i32)]),
    'kvq_bam_to_fastq_host': (i64, [vp, i64, i32, i64, vp, i64, P(i64)]),
    'kvq_bam_to_fastq_device': (i64, [vp, i64, i32, i64, vp, i64, i64, P(BamReport)]),
    'kvq_bam_run_host': (i64, [vp, i64, i64, i32, i64, vp, i64, P(i64)]),
    'kvq_bam_run_device': (i64, [vp, i64, i64, i32, i64, vp, i64, i64, i64, P(i64), P(BamReport)]),
    'kvq_version': (cp, []),
}

_lib = None


def build():
    """compile the library in-tree (hipcc, gfx950)"""
    import subprocess
    subprocess.check_call(['make', '-s', '-C', os.path.join(HERE, 'csrc')])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(PATH):
            raise ImportError('%s is missing: build it with `make -C kvarq_amd/csrc` '
                              '(there is no CPU fallback for the scan)' % PATH)
        L = C.CDLL(PATH)
        for name, (res, args) in PROTOTYPES.items():
            f = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def view(ptr, n, ctype, dtype):
    """numpy view of a C array the library owns (np.ctypeslib.as_array costs ~60 us per call)"""
    addr = C.cast(ptr, C.c_void_p).value
    if not addr or n <= 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((ctype * n).from_address(addr), dtype=dtype)


def kernel_cell(cell):
    """a kvq_scan_kernel_pick / kvq_scan_kernel word as {'k', 'stride', 'lg', 'dense'} (None for 0 = no seed-filter launch)"""
    if cell <= 0:
        return None
    return {'k': cell & 15, 'stride': (cell >> 4) & 15, 'lg': ((cell >> 8) & 15) - 1, 'dense': bool(cell & CELL_DENSE)}


def last_error():
    buf = C.create_string_buffer(1024)
    code = lib().kvq_last_error(buf, 1024)
    return code, buf.value.decode('latin-1')
