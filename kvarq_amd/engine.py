"""
``kvarq.engine`` on an MI355X: the Python module surface of the reference's C
extension (csrc/workhorse.c:1204-1634) -- ``config``, ``get_config``,
``findseqs``, ``stats``, ``stop``, ``test`` and the ``Hit`` namedtuple -- over
the C ABI of libkvarq_hip.so (include/kvarq_hip.h) via ctypes.

Same names, argument meaning, return shapes and exceptions as the reference
(SURVEY.md section 8b).  Strings: file names and sequences may be ``str`` or
``bytes``; ``hitseqs`` come back in the type the sequences were given in
(``str`` via latin-1 for ``str`` input, like the reference under Python 2).

The scan itself runs only on the GPU: without the library or without a device
``findseqs`` raises, it never falls back to a CPU implementation.
"""
import collections
import itertools
import numpy as np
import ctypes as C

from . import _lib
from .fastq import FastqFileFormatException
from .log import lo
from .options import ScanOptions

# workhorse.c:1579-1596
Hit = collections.namedtuple('Hit', 'seq_nr file_pos seq_pos length readlength')
Hit.__doc__ = (
    "seq_nr : refers to the list of sequences in call to engine.findseqs\n"
    "file_pos : beginning of read (within decompressed data)\n"
    "seq_pos : places the beginning of the read relative to the beginning of the sequence\n"
    "length : gives the number of overlapping basepairs\n"
    "readlength : length of the (quality trimmed) read containing the hit\n")

_KEYS = ('maxerrors', 'minoverlap', 'minreadlength', 'nthreads', 'Amin', 'Azero')


def _char(x, name):
    if isinstance(x, str):
        x = x.encode('latin-1')
    if not isinstance(x, (bytes, bytearray)) or len(x) != 1:
        raise TypeError('%s must be a single character' % name)       # format "c", workhorse.c:1503
    v = x[0]
    return v - 256 if v > 127 else v


def config(**kw):
    """config(**kwargs) -- configure the engine (workhorse.c:1498-1507): maxerrors,
    minoverlap, minreadlength, nthreads, Amin, Azero; values persist across calls"""
    for k in kw:
        if k not in _KEYS:
            raise TypeError("'%s' is an invalid keyword argument for this function" % k)
    L = _lib.lib()
    c = _lib.Config()
    L.kvq_config_get(C.byref(c))
    for k in _KEYS[:4]:
        if k in kw:
            if isinstance(kw[k], bool) or not isinstance(kw[k], int):
                raise TypeError('an integer is required')
            setattr(c, k, kw[k])
    for k in _KEYS[4:]:
        if k in kw:
            setattr(c, k, _char(kw[k], k))
    L.kvq_config_set(C.byref(c))


def get_config():
    """get_config() -- the current config as dictionary (workhorse.c:1484-1493)"""
    L = _lib.lib()
    c = _lib.Config()
    L.kvq_config_get(C.byref(c))
    return {'maxerrors': c.maxerrors, 'minoverlap': c.minoverlap, 'minreadlength': c.minreadlength,
            'nthreads': c.nthreads, 'Amin': chr(c.Amin & 0xFF), 'Azero': chr(c.Azero & 0xFF)}


class RescanRequired(MemoryError):
    """kvq_scan_finish after host batches: the hit arena was too small; it has been enlarged, and the same
    batches have to be fed again after a reset (``scan.Scanner`` does that itself)"""


def _raise_last():
    code, msg = _lib.last_error()
    if code == _lib.ERR_FORMAT:
        raise FastqFileFormatException(msg)
    if code == _lib.ERR_IO:
        raise IOError(msg)
    if code == _lib.ERR_RESCAN:
        raise RescanRequired(msg)
    if code == _lib.ERR_MEMORY:
        raise MemoryError(msg)
    if code == _lib.ERR_TYPE:
        raise TypeError(msg)
    raise RuntimeError(msg)


def _stats_dict(readlengths, longest, nseqbasehits, nseqhits, parsed, total, sigints, records):
    # workhorse.c:1205-1244; progress in float32 like the reference (1230-1232)
    progress = 0.0
    if total > 0:
        progress = C.c_float(C.c_float(min(parsed, total)).value / C.c_float(total).value).value
    return {
        'readlengths': tuple(readlengths[i] if i < _lib.MAX_READLENGTH else 0 for i in range(longest + 1)),
        'progress': progress,
        'nseqbasehits': tuple(nseqbasehits),
        'nseqhits': tuple(nseqhits),
        'parsed': parsed, 'total': total, 'sigints': sigints, 'records_parsed': records,
    }


# ---- a finished scan object as Python objects: the one reader of its arrays (findseqs below, scan.Scanner) ----
def scan_arrays(L, h):
    """views of the library's result arrays: the five columns of ``Hit``, 'offsets' (n + 1, into the hit bytes), and the
    hit bytes themselves, 'blob' (``bytes``); valid until the scan object is reset or destroyed"""
    nh = L.kvq_scan_n_hits(h)
    a = {'seq_nr': _lib.view(L.kvq_scan_hit_seq_nr(h), nh, C.c_int32, np.int32), 'file_pos': _lib.view(L.kvq_scan_hit_file_pos(h), nh, C.c_int64, np.int64),
         'seq_pos': _lib.view(L.kvq_scan_hit_seq_pos(h), nh, C.c_int32, np.int32), 'length': _lib.view(L.kvq_scan_hit_length(h), nh, C.c_int32, np.int32),
         'readlength': _lib.view(L.kvq_scan_hit_readlength(h), nh, C.c_int32, np.int32),
         'offsets': _lib.view(L.kvq_scan_hitseq_offsets(h), nh + 1, C.c_int64, np.int64)}
    a['blob'] = C.string_at(L.kvq_scan_hitseq_blob(h), int(a['offsets'][nh])) if nh else b''
    return a


def scan_hits(L, h, as_str=False):
    """-> (the reference's ``hits`` tuple, its ``hitseqs`` list: ``bytes``, or ``str`` via latin-1)"""
    a = scan_arrays(L, h)
    # (the arrays become Python objects in bulk: one ctypes index operation per field of every hit cost more than the scan of a
    # 3 GB file; tuple.__new__(Hit, fields) is what Hit(*fields) ends up calling, without the Python-level frame in between)
    hits = tuple(map(tuple.__new__, itertools.repeat(Hit), zip(*(a[f].tolist() for f in Hit._fields))))
    off, blob = a['offsets'].tolist(), a['blob'].decode('latin-1') if as_str else a['blob']
    return hits, [blob[x:y] for x, y in zip(off, off[1:])]


def scan_records(L, h, as_str=False):
    """the records of a finished scan object's hits, in the order of ``hits`` (kvq_scan_hit_record_off / _len into kvq_scan_record_blob)"""
    nh = L.kvq_scan_n_hits(h)
    if not nh:
        return []
    off = _lib.view(L.kvq_scan_hit_record_off(h), nh, C.c_int64, np.int64).tolist()
    ln = _lib.view(L.kvq_scan_hit_record_len(h), nh, C.c_int32, np.int32).tolist()
    blob = C.string_at(L.kvq_scan_record_blob(h), L.kvq_scan_record_bytes(h))
    if as_str:
        blob = blob.decode('latin-1')
    return [blob[a:a + b] for a, b in zip(off, ln)]


def scan_stats(L, h, nseq, sigints, ctr=None):
    """the ``stats`` dict of a finished scan object over ``nseq`` sequences (``ctr``: its counters, where the caller has them)"""
    # counters layout (include/kvarq_hip.h): 4 scalars, readlengths[1024], nseqhits[n], nseqbasehits[n], ...
    o_hits = _lib.CTR_READLENGTHS + _lib.MAX_READLENGTH
    if ctr is None:
        ctr = _lib.view(L.kvq_scan_counters(h), o_hits + 2 * nseq, C.c_int64, np.int64)
    ctr = ctr[:o_hits + 2 * nseq].tolist()
    return _stats_dict(ctr[_lib.CTR_READLENGTHS:o_hits], ctr[_lib.CTR_LONGEST] - 1, ctr[o_hits + nseq:o_hits + 2 * nseq], ctr[o_hits:o_hits + nseq],
                       L.kvq_scan_parsed(h), L.kvq_scan_total(h), sigints, ctr[_lib.CTR_RECORDS])


_last_inflate = None
_last_long_reads = None
INFLATE_FLAGS = {'host': 0, 'device': 1, 'device_any': 2}     # KVQ_FIND_DEVICE_INFLATE, KVQ_FIND_DEVICE_GZIP
PATH_DEVICE_INFLATE, PATH_DEVICE_GZIP, PATH_DEVICE_BAM = _lib.PATH_DEVICE_INFLATE, _lib.PATH_DEVICE_GZIP, _lib.PATH_DEVICE_BAM


def findseqs(fname, sequences, *, inflate='host', **options):
    """findseqs(fname, sequences) -- finds occurences of base sequences in fastq files
    (workhorse.c:1249-1464).

    fname: file name or sequence of file names (plain or ``.gz``), scanned as one
    stream; sequences: sequence of strings.  Returns ``{'hits': tuple of Hit,
    'stats': dict as stats(), 'hitseqs': list of hit base strings}``.

    inflate='device' (not in the reference): when every file is BGZF (bgzip) to its
    end, the compressed blocks go to the GPU and are inflated, cut and scanned there;
    otherwise the call is the default one.  inflate='device_any': when every file is a
    ``.gz``, each is inflated on the GPU -- a BGZF file by its blocks, any other gzip by
    speculative chunk decoding --; otherwise the call is the default
    one.  last_inflate() tells which route ran, last_inflate_report() what the
    speculative route did.

    records=True (not in the reference): the dict gains 'records', one entry per hit
    (``str`` or ``bytes`` as for 'hitseqs'): the raw bytes of the FastQ record whose
    bases line holds the hit's file_pos, identifier line to quality line, its final
    newline included -- gathered on the GPU during the scan.

    BAM files (not in the reference; recognised by their bytes, not their name) are
    scanned as their *virtual FastQ text* (DESIGN section 12): every primary record with
    bases as '@name[/1|/2]', bases, '+', qualities, the reverse strand restored.  Hits,
    stats, counters and records are those of a scan of that text, and file_pos counts
    its bytes.  The records are decoded on the GPU whatever ``inflate`` says
    (last_inflate() == 'device_bam', last_bam_report() what the route did); a call that
    mixes BAM and other files raises IOError.

    profile=<cutoffs> (not in the reference): the dict gains 'profile', a
    ``kvarq_amd.profile.Profile`` of the whole input -- score and base bytes, read lengths,
    and what the quality trim leaves at each cutoff (characters, bytes or ints, at most 8;
    ``True``: the configured Amin alone) -- taken on the GPU during the scan (DESIGN
    section 13).  ``sequences`` may then be empty.

    cycles=True: that profile also holds the per-cycle counts -- how often every byte stands at
    every position of the score and bases lines (``Profile.cycle_scores`` and what follows it;
    DESIGN section 14).  Without ``profile`` it means a profile with no cutoffs.

    per_read=True / duplication=True: that profile also holds the per-read distributions (GC share,
    mean quality, N count: ``Profile.gc_hist`` and what follows it) / how often the reads' first 64
    bases repeat (``Profile.duplication``).  Without ``profile`` either means a
    profile with no cutoffs.

    overrepresented=True: that profile also lists the sequences (the reads' first 64 bases) that make
    up 0.1 % of the reads and more, among those seen in the first 2^18 records, each counted through
    the whole input (``Profile.overrepresented``).  Without ``profile`` it means a
    profile with no cutoffs.

    adapters=True / {name: bytes} / [bytes, ...]: that profile also tells how much of the input is adapter
    and from which cycle on (``Profile.adapters``): per read and probe the first full
    occurrence of the probe on the bases line, else the longest prefix of the probe (6 bases and more)
    that ends the line, and the histogram of the length an adapter clip would leave.  True: the entries
    of ``profile.KNOWN_SOURCES`` that are bytes.  1 to 8 probes of 8 to 32 upper-case A C G T, matched
    byte for byte.  Without ``profile`` it means a profile with no cutoffs.

    clip=True / {name: bytes} / [bytes, ...] (the forms of ``adapters``; with both, the same probes): adapter
    clipping ahead of the trim.  The score bytes of every record from its adapter's first
    base on -- the ``CLIP`` of the adapter content -- are set to '!' (Phred 0) on the GPU before the batch is
    scanned, so no trimmed read reaches into the adapter: the results are those of a scan of the masked
    text.  The dict gains 'clip' (``profile.Clip``: ``records``, ``clipped``, ``masked``, ``bases_cut``,
    ``words``) and 'clip_kernel_ms'.  It needs no profile; a configured Amin of '!' or below is refused.

    adapter_mismatches=True / 10 .. 32 (with ``adapters`` or ``clip``): the probes of both
    tolerate substitutions -- a comparison over ``len`` bases may differ from the probe in ``len // per``
    positions, True meaning per = 10 (one mismatch in a 12-base probe, none in a tail shorter than 10).  An
    'N', a lower-case letter or any other byte is one mismatch.  The earliest window within the budget is
    the adapter's first base; ``Adapters.first_mismatches`` tells how many of them differed in 0 .. 3 places.
    None, False or 0: the probes match byte for byte, as without the option.

    emit='out.fastq' (not in the reference): the reads as the scan saw them are written to that file as
    FastQ, every file of the call to the one output, in order: every record cut to the part the quality trim leaves of it -- the
    longest run of scores at or above the configured Amin, behind ``clip`` ending in front of the adapter too -- as name, bases,
    a bare '+', scores.  emit_min=N keeps the reads of N bases and more (None: the configured minreadlength; 0 keeps every
    record with matching lines, empty where nothing survives, so that the files of two mates stay in step); records whose bases
    and scores differ in length are dropped.  The compaction runs on the GPU behind the scan.  The dict gains 'emit'
    (``profile.Emit``: ``records``, ``emitted``, ``short``, ``mismatched``, ``bases_in``, ``bases_out``, ``bytes_out``,
    ``words``) and 'emit_kernel_ms'.  It needs no profile.  A call that raises FastqFileFormatException
    raises it as before; what the file holds then is unspecified.

    emit_compress=True beside emit=: the emitted text is deflated on the GPU and the file is BGZF -- what
    ``samtools``, ``bwa`` and ``minimap2`` read as ``.fastq.gz``, and ``findseqs(..., inflate='device')`` too.  The path's suffix
    decides nothing.  The dict gains 'emit_compress' (``members``, ``bytes_in``, ``bytes_out`` without the 28-byte EOF member,
    ``stored``, ``ratio``) and 'emit_deflate_kernel_ms'.  Without emit=: ValueError.

    long_reads=True (not in the reference): the text is scanned on the read-list route (DESIGN section
    15) -- for reads of thousands of bases (PacBio HiFi, nanopore; FastQ or unaligned BAM), which fit
    no tile of the scan kernel and otherwise end in the exhaustive kernels: the seeded sequences are
    found by K-mer lookups over the list of trimmed reads.  The results are the same.  'auto': only the
    batches whose first records average a read of 1024 bases or more take it.  With a sequence list that
    has no seed index the option changes nothing.  last_long_reads() tells whether the route ran."""
    import os, time
    global _last_inflate, _last_long_reads
    opt = ScanOptions(**options)
    if inflate not in INFLATE_FLAGS:
        raise ValueError("inflate must be 'host', 'device' or 'device_any'")
    _last_inflate = _last_long_reads = None
    t_in = time.perf_counter()
    L = _lib.lib()
    if isinstance(fname, (str, bytes)):
        fnames = [fname]
    else:
        try:
            fnames = list(fname)
        except TypeError:
            raise TypeError('fname must be [sequence of] string[s]')              # workhorse.c:1295
    for f in fnames:
        if not isinstance(f, (str, bytes)):
            raise TypeError('fname must be [sequence of] string[s]')
    try:
        seqs = list(sequences)
    except TypeError:
        raise TypeError('seqlist must be sequence of strings')                    # workhorse.c:1302
    as_str = any(isinstance(s, str) for s in seqs) or not seqs and isinstance(fnames[0] if fnames else '', str)
    bseqs = []
    for s in seqs:
        if isinstance(s, str):
            s = s.encode('latin-1')
        elif not isinstance(s, (bytes, bytearray)):
            raise TypeError('seqlist must be list of strings')                    # workhorse.c:1331
        bseqs.append(bytes(s))
    bfiles = [f.encode() if isinstance(f, str) else f for f in fnames]

    n = len(bseqs)
    farr = (C.c_char_p * max(1, len(bfiles)))(*bfiles)
    # sequences may hold NUL bytes: pass raw buffers, not c_char_p strings
    bufs = [C.create_string_buffer(s, len(s) + 1) for s in bseqs]
    sarr = (C.c_char_p * max(1, n))(*[C.cast(b, C.c_char_p) for b in bufs])
    lens = (C.c_int32 * max(1, n))(*[len(s) for s in bseqs])

    # ctypes releases the GIL for the duration of the call (workhorse.c:1377-1408)
    t_0 = time.perf_counter()
    fo = opt.find_opts(INFLATE_FLAGS[inflate])        # (kvq_find_opts, or the longer structure that begins with it)
    h = L.kvq_findseqs_opts(farr, len(bfiles), sarr, lens, n, C.cast(C.byref(fo), C.POINTER(_lib.FindOpts)))
    t_1 = time.perf_counter()
    try:
        if h:
            path = L.kvq_scan_path(h)
            _last_inflate = ('device_bam' if path & PATH_DEVICE_BAM else 'device_gzip' if path & PATH_DEVICE_GZIP
                             else 'device' if path & PATH_DEVICE_INFLATE else 'host')
            _last_long_reads = bool(path & _lib.PATH_READ_LIST)
        code, _ = _lib.last_error()
        if not h or code:
            _raise_last()
        hits, hitseqs = scan_hits(L, h, as_str)
        st = scan_stats(L, h, n, _sigints())
        if os.environ.get('KVQ_TIMING'):
            import sys
            sys.stderr.write('engine.findseqs: arguments %.1f ms, library %.1f ms, results as Python objects %.1f ms\n' % ((t_0 - t_in) * 1e3, (t_1 - t_0) * 1e3, (time.perf_counter() - t_1) * 1e3))
        out = {'hits': hits, 'stats': st, 'hitseqs': hitseqs}
        if _last_inflate == 'device_bam':
            noqual = last_bam_report()['records_noqual']
            if noqual:
                lo.warning('%d BAM records without qualities were written with Phred 1 (\'"\'): at the default Amin '
                           'they are trimmed to nothing' % noqual)
        if opt.records:
            out['records'] = scan_records(L, h, as_str)
        if opt.profile is not None:
            from . import profile as profile_
            out['profile'] = profile_.from_scan(L, h, adapters=(opt.adapter_names, opt.adapters))
        if opt.clip:
            from . import profile as profile_
            out['clip'] = profile_.clip_from_scan(L, h, (opt.clip_names, opt.clip))
            out['clip_kernel_ms'] = L.kvq_scan_clip_kernel_ms(h)
        if opt.emit is not None:
            from . import profile as profile_
            out['emit'] = profile_.emit_from_scan(L, h)
            out['emit_kernel_ms'] = L.kvq_scan_emit_kernel_ms(h)
            if opt.emit_compress:
                out['emit_compress'] = profile_.emit_compress_from_scan(L, h)
                out['emit_deflate_kernel_ms'] = L.kvq_scan_emit_deflate_kernel_ms(h)
        return out
    finally:
        if h:
            t_f = time.perf_counter()
            L.kvq_findseqs_free(h)
            if os.environ.get('KVQ_TIMING'):
                import sys
                sys.stderr.write('engine.findseqs: free %.1f ms\n' % ((time.perf_counter() - t_f) * 1e3))


def last_inflate():
    """where the text of the last findseqs call was inflated: 'device' (the BGZF route on the
    GPU), 'device_gzip' (inflate='device_any' and a file took the speculative route on the GPU),
    'device_bam' (BAM files, decoded to FastQ text on the GPU), 'host' (the reader on the CPU,
    plain files included), or None before any call"""
    return _last_inflate


def last_long_reads():
    """whether a batch of the last findseqs call took the read-list route (``long_reads``); None before any call"""
    return _last_long_reads


def last_bam_report():
    """what the BAM route did in the last call that took it (kvq_bam_report as a dict: runs, segments,
    refuted, check_passes, records_seen / _written / _skipped / _noqual, bam_bytes, text_bytes,
    ms_inflate, ms_find, ms_emit)"""
    rep = _lib.BamReport()
    _lib.lib().kvq_bam_last_report(C.byref(rep))
    return rep.as_dict()


def last_inflate_report():
    """what the speculative gzip route did in the last call that took it (kvq_gzip_report as a dict:
    runs, chunks, candidates_tested, refuted, redecodes, slot_overflows, marker_symbols)"""
    rep = _lib.GzipReport()
    _lib.lib().kvq_gzip_last_report(C.byref(rep))
    return rep.as_dict()


def _sigints():
    L = _lib.lib()
    ls = _lib.LiveStats()
    L.kvq_poll_stats(C.byref(ls), None, None, None, 0)
    return ls.sigints


def stats():
    """stats() -- statistics of the running (or last) scan (workhorse.c:1205-1244);
    may be called from another thread while findseqs runs"""
    L = _lib.lib()
    ls = _lib.LiveStats()
    L.kvq_poll_stats(C.byref(ls), None, None, None, 0)
    n = ls.nseq
    rls = (C.c_int64 * _lib.MAX_READLENGTH)()
    sh = (C.c_int64 * max(1, n))()
    sbh = (C.c_int64 * max(1, n))()
    L.kvq_poll_stats(C.byref(ls), rls, sh, sbh, n)
    return _stats_dict(list(rls), ls.rls_longest, list(sbh)[:n], list(sh)[:n], ls.parsed, ls.total, ls.sigints,
                       ls.records_parsed)


def stop():
    """stop() -- stops the scanning process; findseqs returns the hits found so far
    (workhorse.c:1469-1479)"""
    lo.debug('engine stopped')
    _lib.lib().kvq_request_stop()


def test():
    """test() -- no-op (the reference dumps its disabled profiler, workhorse.c:1512-1517)"""
    return None


def install_sigint_counter():
    """the reference installs, at import, a C SIGINT handler that only counts
    (workhorse.c:133-136, 1632; the CLI turns two of them into stop(), cli.py:156-164).
    Replacing the process's handler is a process-wide side effect, so here it is an
    explicit call: the ``kvarq/engine.py`` shim of INTEGRATION.md makes it.  The handler
    lives in the library (``kvq_sigint_counter_install``): it counts while the main
    thread is inside ``findseqs``, where a Python-level handler would have to wait."""
    if _lib.lib().kvq_sigint_counter_install():
        _raise_last()


def remove_sigint_counter():
    """puts back the handler that was there before ``install_sigint_counter``"""
    _lib.lib().kvq_sigint_counter_remove()
