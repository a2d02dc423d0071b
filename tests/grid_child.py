"""
Child program of tests/test_gpu_kernel_matrix.py (not a test): scans texts in a process of its own, because the
switches of the launcher (KVQ_GRID among them) are read once per process.  The parent sets the environment; this
program sets none, and it never sees the oracle: it only writes down what the library gave.

    python grid_child.py JOB.json

JOB.json: {"texts": [files of raw FastQ text], "seqs": [sequences, latin-1], "cfg": {engine configuration},
"result": file}.  The result is an .npz with, for text i, ``t<i>_<name>``: the five hit columns (seq_nr, file_pos,
seq_pos, length, readlength), the hit bytes (blob) and their offsets, nseqhits, nseqbasehits, readlengths,
records_parsed, coverage, mutations, and kernel, path and grid as one JSON string (meta).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(job_path):
    from kvarq_amd import scan
    with open(job_path) as f:
        job = json.load(f)
    t = scan.Table([q.encode('latin-1') for q in job['seqs']], **job['cfg'])
    out = {}
    for i, path in enumerate(job['texts']):
        text = np.fromfile(path, dtype=np.uint8)
        s = scan.Scanner(t)
        s.scan_host(text)
        r = s.finish()
        s.close()
        hits, st = r['hits'], r['stats']
        for c, name in enumerate(('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')):
            out['t%d_%s' % (i, name)] = np.array([h[c] for h in hits], dtype=np.int64)
        out['t%d_blob' % i] = np.frombuffer(b''.join(r['hitseqs']), dtype=np.uint8)
        out['t%d_offsets' % i] = np.cumsum([0] + [len(b) for b in r['hitseqs']], dtype=np.int64)
        for name in ('nseqhits', 'nseqbasehits', 'readlengths'):
            out['t%d_%s' % (i, name)] = np.array(st[name], dtype=np.int64)
        out['t%d_records_parsed' % i] = np.array(st['records_parsed'], dtype=np.int64)
        out['t%d_coverage' % i] = np.array(r['coverage'], dtype=np.int64)
        out['t%d_mutations' % i] = np.array(r['mutations'], dtype=np.int64)
        out['t%d_meta' % i] = np.array(json.dumps(dict(kernel=r['kernel'], path=r['path'], grid=r['grid'])))
    t.close()
    with open(job['result'], 'wb') as f:
        np.savez(f, **out)
    print('grid child ok: %d texts' % len(job['texts']))


if __name__ == '__main__':
    main(sys.argv[1])
