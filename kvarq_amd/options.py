"""
The options of a scan that are not in the reference -- ``records``, ``profile``, ``cycles``, ``long_reads``, ``per_read``,
``duplication``, ``overrepresented``, ``adapters``, ``clip``, ``adapter_mismatches``, ``emit``, ``emit_min``, ``emit_compress`` -- said once: ``engine.findseqs`` and ``scan.Scanner`` take them as ``**options`` and normalise them here, and
everything that passes a scan on (``Analyser.scan``, ``Fastq.profile``, ``Bam.profile``, ``profile.profile``) forwards them.
"""
import ctypes as C
import operator

from . import _lib


def as_mismatch_per(adapter_mismatches):
    """the ``per`` of kvq_scan_set_adapter_mismatches for an ``adapter_mismatches`` option: None, False or 0 -> 0 (exact), True -> 10,
    an int 10 .. 32 -> itself"""
    if adapter_mismatches is None or adapter_mismatches is False:
        return 0
    if adapter_mismatches is True:
        return 10
    try:
        per = operator.index(adapter_mismatches)             # (any integer type, numpy's among them; no float, no string)
    except TypeError:
        per = -1
    if not (per == 0 or 10 <= per <= 32):
        raise ValueError('adapter_mismatches is None, False or 0 (exact), True (10) or an int 10 .. 32: one mismatch per that many bases')
    return per


def as_emit(emit, emit_min=None):
    """``(emit, min_length)`` for an ``emit`` and an ``emit_min`` option.  ``emit``: None or False -> None (off); True -> True (the
    emitted text is handed back); a path (str, bytes, os.PathLike) -> its bytes (the text is streamed there).  ``emit_min``: None ->
    -1 (the configured minreadlength); an int >= 0 -> itself; anything else, or an ``emit_min`` without ``emit``: ValueError"""
    import os
    if emit is None or emit is False:
        emit = None
    elif emit is not True:
        try:
            emit = os.fsencode(emit)
        except TypeError:
            raise ValueError('emit is None or False (off), True, or the path of the output')
        if not emit:
            raise ValueError('emit is None or False (off), True, or the path of the output')
    if emit_min is None:
        return emit, -1
    try:
        m = -1 if isinstance(emit_min, bool) else operator.index(emit_min)
    except TypeError:
        m = -1
    if m < 0 or m > 0x7FFFFFFF:
        raise ValueError('emit_min is None (the configured minreadlength) or an int >= 0')
    if emit is None:
        raise ValueError('emit_min= is the shortest read emit= keeps: give emit= too')
    return emit, m


def as_emit_compress(emit_compress, emit):
    """the ``emit_compress`` option beside a normalised ``emit``: None or False -> False; True -> True; anything else, and True
    without ``emit``: ValueError"""
    if emit_compress is None:
        return False
    if not isinstance(emit_compress, bool):
        raise ValueError('emit_compress is a bool')
    if emit_compress and emit is None:
        raise ValueError('emit_compress= is the form of what emit= writes: give emit= too')
    return emit_compress


class ScanOptions(object):
    """``records``: keep the FastQ record of every hit; ``profile``: the cutoffs of the input's profile
    (``profile.as_cutoffs``; True: ``amin``, or the configured Amin; None: no profile) -- a list of byte values here;
    ``cycles``: the per-cycle counts beside it; ``read_stats``: the mode bits of kvq_scan_set_read_stats for ``per_read`` and
    ``duplication``; ``overrepresented``: the overrepresented sequences; ``long_mode``: the mode of kvq_scan_set_long_reads
    for ``long_reads`` (False, True or 'auto'); ``adapters``: the probes of the adapter content (``profile.as_adapters``: True,
    a mapping name -> bytes or a list of bytes; None or False: off) -- ``adapter_names`` and ``adapters``, a list of bytes, here.
    ``cycles``, ``per_read``, ``duplication``, ``overrepresented`` or ``adapters`` without ``profile`` mean a profile with no cutoffs.
    ``clip``: the probes of the adapter clip ahead of the trim, in the forms of ``adapters`` -- ``clip_names`` and
    ``clip``, a list of bytes, here; it needs no profile.  ``adapters`` and ``clip`` together must name the same probes (``findseqs``
    has one probe block): otherwise ValueError.  ``adapter_mismatches``: the probes of both tolerate one mismatch per that many bases
     -- None, False or 0: exact; True: 10; an int 10 .. 32 as given -- ``mismatch_per``, an int, here; without
    ``adapters`` or ``clip``, and outside the range: ValueError.
    ``emit``: the reads the scan saw, as FastQ text -- None or False: off; True: handed back (``Scanner``); a path:
    streamed there (``findseqs`` takes nothing else) -- True or the path's bytes here; ``emit_min``: the shortest read it keeps -- None:
    the configured minreadlength, -1 here; an int >= 0 as given; anything else, and without ``emit``: ValueError (``as_emit``).  It
    needs no profile.  ``emit_compress``: the emitted text leaves the GPU as BGZF, deflated there -- a bool;
    anything else, and True without ``emit``: ValueError.  The path's suffix decides nothing."""

    def __init__(self, records=False, profile=None, cycles=False, long_reads=False, per_read=False, duplication=False, overrepresented=False,
                 adapters=None, clip=None, amin=None, adapter_mismatches=None, emit=None, emit_min=None, emit_compress=None):
        self.emit, self.emit_min = as_emit(emit, emit_min)
        self.emit_compress = as_emit_compress(emit_compress, self.emit)
        self.long_reads, self.long_mode = long_reads, _lib.long_reads_mode(long_reads)
        self.records, self.cycles, self.overrepresented = bool(records), bool(cycles), bool(overrepresented)
        self.read_stats = (_lib.READ_STATS if per_read else 0) | (_lib.READ_DUPLICATION if duplication else 0)
        self.adapter_names, self.adapters = None, None
        if adapters is not None and adapters is not False:
            from .profile import as_adapters
            self.adapter_names, self.adapters = as_adapters(adapters)
        self.clip_names, self.clip = None, None
        if clip is not None and clip is not False:
            from .profile import as_adapters
            self.clip_names, self.clip = as_adapters(clip)
            if self.adapters and self.adapters != self.clip:
                raise ValueError('adapters= and clip= must name the same probes')
            # (where the caller knows the table's Amin: what kvq_scan_set_clip refuses, refused before a scan object is made)
            a = None if amin is None else amin & 0xFF if isinstance(amin, int) else (amin.encode('latin-1') if isinstance(amin, str) else bytes(amin))[0]
            if a is not None and (a ^ 0x80) - 0x80 <= ord('!'):
                raise ValueError("clip= needs an Amin above '!': a masked score would end no run")
        self.mismatch_per = as_mismatch_per(adapter_mismatches)
        if self.mismatch_per and not (self.adapters or self.clip):
            raise ValueError('adapter_mismatches= is the rule of the probes of adapters= or clip=: give one of them')
        if (self.cycles or self.read_stats or self.overrepresented or self.adapters) and profile is None:
            profile = ()
        self.profile = None
        if profile is not None:
            from .profile import as_cutoffs
            self.profile = as_cutoffs(profile, amin=amin)

    def find_opts(self, flags=0):
        """the kvq_find_opts of kvq_findseqs_opts (``flags``: the caller's own, OR-ed in)"""
        flags |= (0, _lib.FIND_LONG_READS, _lib.FIND_LONG_READS_AUTO)[self.long_mode] | (_lib.FIND_RECORDS if self.records else 0)
        if self.profile is not None:
            flags |= (_lib.FIND_PROFILE | (_lib.FIND_CYCLES if self.cycles else 0) | (_lib.FIND_READ_STATS if self.read_stats & _lib.READ_STATS else 0) |
                      (_lib.FIND_DUPLICATION if self.read_stats & _lib.READ_DUPLICATION else 0) | (_lib.FIND_OVERREPRESENTED if self.overrepresented else 0))
        cuts = self.profile or ()
        base = _lib.FindOpts(C.sizeof(_lib.FindOpts), flags, len(cuts), (C.c_uint8 * 8)(*cuts))
        probes = self.adapters or self.clip
        if not probes:
            return self._with_emit(base)
        # (the probes ride behind the 20 bytes, which stay what they are whenever the adapters and the clip are off)
        base.size, base.flags = C.sizeof(_lib.FindOptsAdapters), flags | (_lib.FIND_ADAPTERS if self.adapters else 0) | (_lib.FIND_CLIP if self.clip else 0)
        o = _lib.FindOptsAdapters(base, len(probes), (C.c_uint8 * 8)(*[len(p) for p in probes]))
        for k, p in enumerate(probes):
            C.memmove(o.probes[k], p, len(p))
        if not self.mismatch_per:
            return self._with_emit(o)
        # (the rate rides behind the probes, which stay what they are whenever it is off)
        o.base.size, o.base.flags = C.sizeof(_lib.FindOptsAdaptersMm), o.base.flags | _lib.FIND_ADAPTER_MISMATCHES
        return self._with_emit(_lib.FindOptsAdaptersMm(o, self.mismatch_per))

    def _with_emit(self, o):
        """``o``, or with ``emit`` the kvq_find_opts_emit that begins with it: min_length and the path ride behind everything else, and
        the blocks in front that ``o`` does not have stay zero (they are read only under their own flags)"""
        if self.emit is None:
            return o
        if self.emit is True:
            raise ValueError('findseqs streams the emitted reads to a file: emit= is the path of the output')
        if isinstance(o, _lib.FindOpts):
            o = _lib.FindOptsAdapters(o)
        if isinstance(o, _lib.FindOptsAdapters):
            o = _lib.FindOptsAdaptersMm(o, 0)
        e = _lib.FindOptsEmit(o, self.emit_min, self.emit)
        e.m.a.base.size, e.m.a.base.flags = C.sizeof(_lib.FindOptsEmit), e.m.a.base.flags | _lib.FIND_EMIT | (_lib.FIND_EMIT_BGZF if self.emit_compress else 0)
        return e

    def setters(self):
        """the kvq_scan_set_* calls of a new scan handle, in order: (name, arguments behind the handle)"""
        calls = [('kvq_scan_set_records', (1,))] if self.records else []
        if self.profile is not None:
            calls.append(('kvq_scan_set_profile', ((C.c_uint8 * 8)(*self.profile), len(self.profile))))
            if self.cycles:
                calls.append(('kvq_scan_set_cycles', (1,)))
            if self.read_stats:
                calls.append(('kvq_scan_set_read_stats', (self.read_stats,)))
            if self.overrepresented:
                calls.append(('kvq_scan_set_overrepresented', (1,)))
            if self.adapters:
                n = len(self.adapters)
                calls.append(('kvq_scan_set_adapters', ((C.c_char_p * n)(*self.adapters), (C.c_int32 * n)(*[len(p) for p in self.adapters]), n)))
        if self.clip:
            n = len(self.clip)
            calls.append(('kvq_scan_set_clip', ((C.c_char_p * n)(*self.clip), (C.c_int32 * n)(*[len(p) for p in self.clip]), n)))
        if self.mismatch_per:
            calls.append(('kvq_scan_set_adapter_mismatches', (self.mismatch_per,)))
        if self.long_mode:
            calls.append(('kvq_scan_set_long_reads', (self.long_mode,)))
        if self.emit is not None:
            calls.append(('kvq_scan_set_emit', (1, self.emit_min)))      # (a path: the caller opens it and hands it over, kvq_scan_set_emit_fd)
            if self.emit_compress:
                calls.append(('kvq_scan_set_emit_compress', (1,)))
        return calls
