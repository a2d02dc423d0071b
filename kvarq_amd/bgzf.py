"""
BGZF (bgzip) members as the library sees them: the block index of a file's bytes and the
library's own raw-DEFLATE decoder run on the host (include/kvarq_hip.h, kvq_bgzf_index and
kvq_inflate_raw_host).  The decoder is the one the GPU runs (kvarq_amd.scan.inflate_bgzf_device);
on the host it is for tests and for looking at a member that failed.
"""
import ctypes as C

import numpy as np

from . import _lib

Z_OK, Z_STREAM_ERROR, Z_DATA_ERROR, Z_BUF_ERROR = 0, -2, -3, -5


def index(data):
    """(block offsets, block bytes, isizes) as int64/uint32/uint32 arrays, or None when the bytes are not BGZF to the end"""
    data = bytes(data)
    L = _lib.lib()
    n = L.kvq_bgzf_index(data, len(data), None, None, None, 0)
    if n < 0:
        return None
    off = np.zeros(max(1, n), np.int64)
    cs = np.zeros(max(1, n), np.uint32)
    isz = np.zeros(max(1, n), np.uint32)
    L.kvq_bgzf_index(data, len(data), off.ctypes.data_as(C.POINTER(C.c_int64)), cs.ctypes.data_as(C.POINTER(C.c_uint32)),
                     isz.ctypes.data_as(C.POINTER(C.c_uint32)), n)
    return off[:n], cs[:n], isz[:n]


def payload(data, off, csize):
    """the raw DEFLATE payload of the block at `off` (between its header and its CRC32/ISIZE trailer)"""
    off, csize = int(off), int(csize)
    xlen = data[off + 10] | data[off + 11] << 8
    return bytes(data[off + 12 + xlen:off + csize - 8])


def inflate_raw_host(payload, isize):
    """(status, bytes): status 0 and exactly isize bytes, or a negative zlib status and None"""
    payload = bytes(payload)
    isize = int(isize)
    out = C.create_string_buffer(max(1, isize))
    st = _lib.lib().kvq_inflate_raw_host(payload, len(payload), out, isize)
    return st, (out.raw[:isize] if st == Z_OK else None)
