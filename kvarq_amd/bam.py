"""
BAM input (include/kvarq_hip.h, kvq_bam_*): ``engine.findseqs`` scans a BAM file
as its *virtual FastQ text* -- every primary record with bases, ``'@' name ['/1'|'/2'] '\\n' bases
'\\n+\\n' qualities '\\n'``, the reverse strand restored -- decoded on the GPU.  This module holds
what a caller needs around that: recognising a BAM, its header, the virtual text of inflated BAM
bytes on the CPU (the twin of the GPU route) and on the GPU (the route's kernels alone), and
:class:`Bam`, which ``Analyser.scan`` takes in place of a ``Fastq``.
"""
import ctypes as C
import gzip
import os
import struct
import zlib

from . import _lib
from .fastq import ASCII, Fastq, FastqFileFormatException
from .log import lo


class BamError(IOError):
    """a malformed BAM header or record (the message of the route: "malformed BAM record : offset=<o>")"""


def _first_block_payload(fd):
    """the DEFLATE payload of the BGZF block at the front of a file (None when there is none)"""
    h = fd.read(12)
    if len(h) < 12 or h[:4] != b'\x1f\x8b\x08\x04':
        return None
    xlen = struct.unpack('<H', h[10:12])[0]
    x = fd.read(xlen)
    bsize, i = None, 0
    while i + 4 <= len(x):
        slen = struct.unpack('<H', x[i + 2:i + 4])[0]
        if x[i:i + 2] == b'BC' and slen == 2 and i + 6 <= len(x):
            bsize = struct.unpack('<H', x[i + 4:i + 6])[0] + 1
        i += 4 + slen
    if bsize is None or bsize < 12 + xlen + 8:
        return None
    return fd.read(bsize - 12 - xlen - 8)


def is_bam(path):
    """does the file start with a BGZF block whose inflated bytes begin with ``BAM\\1``?  (the rule of the route; the name
    does not matter, and only the magic is inflated)"""
    try:
        with open(path, 'rb') as fd:
            payload = _first_block_payload(fd)
    except OSError:
        return False
    if payload is None:
        return False
    try:
        return zlib.decompressobj(-15).decompress(payload, 4) == b'BAM\x01'
    except zlib.error:
        return False


def inflate(path):
    """the whole inflated stream of a BAM file (header included), on the CPU"""
    with open(path, 'rb') as fd:
        return gzip.decompress(fd.read())


def _header(data):
    n_ref = C.c_int32(0)
    first = _lib.lib().kvq_bam_header_host(data, len(data), C.byref(n_ref))
    return first, n_ref.value


def header(path):
    """{'n_ref', 'first_record', 'text'}: the header of a BAM file (kvq_bam_header_host over its leading blocks)"""
    with gzip.open(path, 'rb') as fd:
        data = b''
        while True:
            more = fd.read(1 << 16)
            data += more
            first, n_ref = _header(data)
            if first >= 0:
                l_text = struct.unpack('<i', data[4:8])[0]
                return {'n_ref': n_ref, 'first_record': first, 'text': data[8:8 + l_text]}
            if first == -1 or not more:
                raise BamError('malformed BAM header')


def last_report():
    """kvq_bam_last_report as a dict (engine.last_bam_report)"""
    rep = _lib.BamReport()
    _lib.lib().kvq_bam_last_report(C.byref(rep))
    return rep.as_dict()


def _raise():
    code, msg = _lib.last_error()
    raise BamError(msg) if code == _lib.ERR_IO else RuntimeError(msg)


def to_fastq_host(data):
    """the virtual FastQ text of a BAM file's inflated bytes (header included), by kvq_bam_to_fastq_host"""
    data = bytes(data)
    first, n_ref = _header(data)
    if first < 0:
        raise BamError('malformed BAM header')
    L = _lib.lib()
    consumed = C.c_int64(0)
    n = L.kvq_bam_to_fastq_host(data, len(data), n_ref, first, None, 0, C.byref(consumed))
    if n < 0:
        _raise()
    out = C.create_string_buffer(max(1, n))
    L.kvq_bam_to_fastq_host(data, len(data), n_ref, first, out, n, C.byref(consumed))
    return out.raw[:n]


def to_fastq_device(data, segment_bytes=None):
    """the same by the GPU route's kernels (kvq_bam_to_fastq_device); segment_bytes None: KVQ_BAM_SEGMENT_KB"""
    data = bytes(data)
    first, n_ref = _header(data)
    if first < 0:
        raise BamError('malformed BAM header')
    L = _lib.lib()
    d_in = L.kvq_device_alloc(max(1, len(data)))
    d_out = None
    try:
        if not d_in or L.kvq_memcpy_h2d(d_in, data, len(data)):
            raise RuntimeError('device memory')
        sb = int(segment_bytes or 0)
        n = L.kvq_bam_to_fastq_device(d_in, len(data), n_ref, first, None, 0, sb, None)
        if n < 0:
            _raise()
        d_out = L.kvq_device_alloc(max(1, n))
        if not d_out:
            raise RuntimeError('device memory')
        if L.kvq_bam_to_fastq_device(d_in, len(data), n_ref, first, d_out, n, sb, None) != n:
            _raise()
        out = C.create_string_buffer(max(1, n))
        if n and L.kvq_memcpy_d2h(out, d_out, n):
            raise RuntimeError('device copy')
        return out.raw[:n]
    finally:
        if d_in:
            L.kvq_device_free(d_in)
        if d_out:
            L.kvq_device_free(d_out)


def run_host(data, n, n_ref, first_record, limit=None):
    """one run as the route takes it (kvq_bam_run_host): ``data[:n]`` is a prefix of a stream that ends at ``limit``
    (None: ``len(data)``).  Returns (text, end): the text of the records wholly inside the prefix, and where the chain
    left it.  BamError at a malformed record."""
    data = bytes(data)
    limit = len(data) if limit is None else limit
    L = _lib.lib()
    end = C.c_int64(-1)
    t = L.kvq_bam_run_host(data, n, limit, n_ref, first_record, None, 0, C.byref(end))
    if t < 0:
        _raise()
    out = C.create_string_buffer(max(1, t))
    if L.kvq_bam_run_host(data, n, limit, n_ref, first_record, out, t, C.byref(end)) != t:
        _raise()
    return out.raw[:t], end.value


def run_device(d_p, n, limit, n_ref, first_record, d_out, out_off, cap, segment_bytes=None):
    """kvq_bam_run_device on buffers the caller holds in device memory (kvq_device_alloc).  Returns (text bytes, end,
    report dict); BamError at a malformed record (``.end`` and ``.report`` on the exception)."""
    end = C.c_int64(-1)
    rep = _lib.BamReport()
    t = _lib.lib().kvq_bam_run_device(d_p, n, limit, n_ref, first_record, d_out, out_off, cap, int(segment_bytes or 0),
                                      C.byref(end), C.byref(rep))
    if t < 0:
        try:
            _raise()
        except BamError as e:
            e.end, e.report = end.value, rep.as_dict()
            raise
    return t, end.value, rep.as_dict()


def _first_written_length(path):
    """l_seq of the first record that writes text (0 when there is none), read record by record from the front"""
    with gzip.open(path, 'rb') as fd:
        data = b''
        while True:
            more = fd.read(1 << 16)
            data += more
            first, _ = _header(data)
            if first >= 0 or first == -1 or not more:
                break
        if first < 0:
            raise BamError('malformed BAM header')
        o = first
        while True:
            while len(data) < o + 36:
                more = fd.read(1 << 16)
                if not more:
                    return 0
                data += more
            bs, = struct.unpack('<i', data[o:o + 4])
            flag, l_seq = struct.unpack('<Hi', data[o + 18:o + 24])
            if not flag & 0x900 and l_seq > 0:
                return l_seq
            o += 4 + bs


class Bam(object):
    """a BAM file where ``Analyser.scan`` takes a :class:`kvarq_amd.fastq.Fastq`: the scan reads the virtual FastQ text,
    whose qualities are Phred + 33 (the Sanger scale: ``dQ`` 0 in ``Fastq``'s terms, the offset of Q = 0 in ``ASCII``, so
    that ``Azero`` is '!').  ``extract_hits`` needs ``scan(..., records=True)``: there is no file to seek in."""

    ASCII = ASCII

    def __init__(self, fname, quiet=False):
        if not is_bam(fname):
            raise FastqFileFormatException('not a BAM file: "%s"' % fname)
        self.fname, self.fname2, self.gz = fname, None, True
        self.variants, self.dQ = ['Sanger'], Fastq.vendor_variants['Sanger'].dQ
        self.Azero = ASCII[self.dQ]
        self.readlength = _first_written_length(fname)
        self.records_approx = None
        if not quiet:
            lo.info('bam : readlength=%d dQ=%d variants=%s' % (self.readlength, self.dQ, self.variants))

    def filenames(self):
        return [self.fname]

    def filesizes(self):
        return [os.path.getsize(f) for f in self.filenames()]

    def A2Q(self, A):
        return ASCII.index(A) - self.dQ

    def Q2A(self, Q):
        return ASCII[Q + self.dQ]

    def profile(self, cutoffs=None, **options):
        """a ``kvarq_amd.profile.Profile`` of the file's virtual FastQ text, taken on the GPU; cutoffs None: the
        configured Amin; ``cycles``: with the per-cycle counts; ``long_reads``: as for ``engine.findseqs``
        (``options``: as for ``kvarq_amd.profile.profile``)"""
        from . import profile as profile_
        return profile_.profile(self.filenames(), True if cutoffs is None else cutoffs, **options)

    def readrecordat(self, hit):
        raise IOError('the records of a BAM file are kept by the scan only: use Analyser.scan(..., records=True) '
                      'before extract_hits')

