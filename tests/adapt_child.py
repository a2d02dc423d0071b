"""
Child program of tests/test_gpu_adapt.py (not a test): scans one text with the adapter content in a process of its own, because
KVQ_ARENA_CAP is read when a scan object is made and the parent's process may hold kept ones.  The parent sets the environment;
this program sets none and compares nothing: it only writes down what the library gave.

    python adapt_child.py JOB.json

JOB.json: {"text": file of raw FastQ text, "seqs": [sequences, latin-1], "cfg": {engine configuration}, "probes": [probes,
latin-1], "how": "host" | "device", "result": file}.  The result is an .npz with the adapter array (adapt), the profile's words
(words), n_hits and the record counter (records).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(job_path):
    from kvarq_amd import _lib, scan
    with open(job_path) as f:
        job = json.load(f)
    t = scan.Table([q.encode('latin-1') for q in job['seqs']], **job['cfg'])
    text = np.fromfile(job['text'], dtype=np.uint8)
    s = scan.Scanner(t, profile=[], adapters=[p.encode('latin-1') for p in job['probes']])
    if job['how'] == 'host':
        s.scan_host(text)
    else:
        d = scan.DeviceBuffer(text.nbytes); d.upload(text)
        s.scan_device(d.ptr, text.nbytes, scan.chunk_offsets(text))
    r = s.finish(hits=False)
    s.close(); t.close()
    with open(job['result'], 'wb') as f:
        np.savez(f, adapt=r['profile'].adapters.words, words=r['profile'].words, n_hits=np.array(r['n_hits'], dtype=np.int64),
                 records=np.array(r['counters'][_lib.CTR_RECORDS], dtype=np.int64))
    print('adapt child ok')


if __name__ == '__main__':
    main(sys.argv[1])
