"""
Plain gzip inflated by speculative chunk decoding (include/kvarq_hip.h,
kvq_inflate_gzip_host).  The same decoder source and chunked algorithm the GPU runs
(kvarq_amd.scan.inflate_gzip_device), on the CPU: for tests and for looking at a stream.
"""
import ctypes as C

import numpy as np

from . import _lib


class GzipError(IOError):
    """the DEFLATE data do not inflate: .status (zlib's), .fpos (text offset of the failing block's output)"""

    def __init__(self, msg, status, fpos):
        super().__init__(msg)
        self.status, self.fpos = status, fpos


def _call(fn, src, n, chunk_bytes, out_cap, out_ptr):
    st, fp, rep = C.c_int32(0), C.c_int64(-1), _lib.GzipReport()
    got = fn(src, n, int(chunk_bytes), out_ptr, out_cap, C.byref(st), C.byref(fp), C.byref(rep))
    if got == -1:
        raise GzipError(_lib.last_error()[1], st.value, fp.value)
    if got < 0:
        raise IOError(_lib.last_error()[1])
    return got, rep.as_dict()


def inflate_host(data, chunk_bytes):
    """(text, report) of a whole gzip file's bytes, by kvq_inflate_gzip_host; GzipError / IOError as the host route raises"""
    data = bytes(data)
    cap = max(1 << 16, 4 * len(data))
    while True:
        out = C.create_string_buffer(cap)
        got, rep = _call(_lib.lib().kvq_inflate_gzip_host, data, len(data), chunk_bytes, cap, out)
        if got <= cap:
            return out.raw[:got], rep
        cap = got


def last_report():
    rep = _lib.GzipReport()
    _lib.lib().kvq_gzip_last_report(C.byref(rep))
    return rep.as_dict()


def last_chunks():
    """(candidates per nominal chunk start, chunk start bits, chunk end bits, chunk symbols) of the last in-memory call"""
    L = _lib.lib()
    nc = C.c_int64(0)
    m = L.kvq_gzip_last_chunks(None, 0, None, None, None, 0, C.byref(nc))
    cand = np.zeros(max(1, nc.value), np.int64)
    st, en, ns = (np.zeros(max(1, m), np.int64) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    L.kvq_gzip_last_chunks(p(cand), nc.value, p(st), p(en), p(ns), m, C.byref(nc))
    return cand[:nc.value], st[:m], en[:m], ns[:m]


def slot_canaries(pad_symbols):
    """test hook: pad every chunk slot from now on with pad_symbols canary symbols a side (0: off); returns the canary
    symbols found overwritten since the last call"""
    return _lib.lib().kvq_gzip_slot_canaries(int(pad_symbols))
