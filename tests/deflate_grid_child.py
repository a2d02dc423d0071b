"""
The child of tests/test_gpu_deflate.py::test_where_one_workgroup_walks_all_the_tiles: KVQ_GRID is read once per process, so the scan
under it runs here.  ``deflate_grid_child.py TEXT RESULT``: scans TEXT (tests/clip_ref.py's `reveal`, its table and config) as one
host batch with the emit and its deflate on and writes what it got to RESULT (npz): the compressed stream, the emit's and the
deflate's words, the guards' count, the hits' file_pos, the grid of the seed-filter launch and whether it ran.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import clip_ref as CR                                   # noqa: E402
import emit_ref as E                                    # noqa: E402
from kvarq_amd import _lib, scan                        # noqa: E402
from oracle import oracle as O                          # noqa: E402


def main(text_path, result):
    with open(text_path, 'rb') as f:
        text = f.read()
    t = scan.Table(list(CR.TM.table()), **E.CFG)
    s = scan.Scanner(t, emit=True, emit_compress=True)
    s.scan_host(np.frombuffer(text, dtype=np.uint8), chunk_off=list(O.chunk_offsets(text)))
    r = s.finish()
    np.savez(result, emitted=r['emitted'], words=r['emit'].words, zwords=r['emit_compress']['words'], guard=_lib.lib().kvq_scan_emit_guard(s.h),
             grid=r['grid'], seeded=r['path']['seeded'], file_pos=np.array([h.file_pos for h in r['hits']], dtype=np.int64))
    s.close(); t.close()
    print('deflate grid child ok')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
