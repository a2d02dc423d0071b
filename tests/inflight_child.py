"""
Child program of tests/test_gpu_inflight.py (not a test): scans in a process of its own, because KVQ_SV_MODE, KVQ_SV_GRID and
KVQ_GRID are read once per process (and KVQ_SURV_CAP / KVQ_ARENA_CAP when a scan object is made).  The parent sets the
environment; this program sets none, and it never sees the oracle: it only writes down what the library gave.

    python inflight_child.py JOB.json

JOB.json, kind "rounds": {"groups": [{"seqs": [latin-1], "cfg": {...}, "texts": [files of raw FastQ text]}], "result": file}.
Every group has a table and ONE scanner, reset between its texts; a text is one device batch.
Kind "ring": {"tables": [{"seqs", "cfg", "options": {Scanner options}}], "texts": [files], "steps": K, "depth": D, "result": file}.
Scanner i scans with table i; step k resets scanner k % D, hands it text (k + k // D) % len(texts) as two device batches cut at a
chunk offset (the second one's pointer aligned down to 16 bytes) and calls finish_begin; D steps are in flight -- bench.py's loop.

The result is an .npz with, under ``<prefix>_<name>`` (prefix g<group>t<text> or s<step>): the five hit columns, the hit bytes and
their offsets, nseqhits, nseqbasehits, readlengths, records_parsed, coverage, mutations, and one JSON string (meta): kernel, path,
grid, launch_info, and for "rounds" match_info and order_info; for a scanner with records their bytes and offsets, with a profile
its words and cutoffs.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def pack(out, prefix, r, meta):
    hits, st = r['hits'], r['stats']
    for c, name in enumerate(('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')):
        out['%s_%s' % (prefix, name)] = np.array([h[c] for h in hits], dtype=np.int64)
    out[prefix + '_blob'] = np.frombuffer(b''.join(r['hitseqs']), dtype=np.uint8)
    out[prefix + '_offsets'] = np.cumsum([0] + [len(b) for b in r['hitseqs']], dtype=np.int64)
    for name in ('nseqhits', 'nseqbasehits', 'readlengths'):
        out['%s_%s' % (prefix, name)] = np.array(st[name], dtype=np.int64)
    out[prefix + '_records_parsed'] = np.array(st['records_parsed'], dtype=np.int64)
    out[prefix + '_coverage'] = np.array(r['coverage'], dtype=np.int64)
    out[prefix + '_mutations'] = np.array(r['mutations'], dtype=np.int64)
    if 'records' in r:
        out[prefix + '_rec_blob'] = np.frombuffer(b''.join(r['records']), dtype=np.uint8)
        out[prefix + '_rec_offsets'] = np.cumsum([0] + [len(b) for b in r['records']], dtype=np.int64)
    if 'profile' in r:
        out[prefix + '_profile'] = np.array(r['profile'].words, dtype=np.int64)
        out[prefix + '_profile_cutoffs'] = np.frombuffer(bytes(r['profile'].cutoffs), dtype=np.uint8)
    out[prefix + '_meta'] = np.array(json.dumps(dict(meta, kernel=r['kernel'], path=r['path'], grid=r['grid'])))


def rounds(job, out):
    from kvarq_amd import scan
    for gi, group in enumerate(job['groups']):
        t = scan.Table([q.encode('latin-1') for q in group['seqs']], **group['cfg'])
        s = scan.Scanner(t)
        for ti, path in enumerate(group['texts']):
            text = np.fromfile(path, dtype=np.uint8)
            d = scan.DeviceBuffer(text.nbytes); d.upload(text)
            s.reset()
            cap0 = s.order_info()['arena_cap']
            s.scan_device(d.ptr, text.nbytes, scan.chunk_offsets(text))
            r = s.finish()
            pack(out, 'g%dt%d' % (gi, ti), r, dict(launch_info=s.launch_info(), match_info=s.match_info(), order_info=s.order_info(), arena_cap_before=cap0))
            d.free()
        s.close(); t.close()


def ring(job, out):
    from kvarq_amd import scan
    import inflight as F
    tables = [scan.Table([q.encode('latin-1') for q in tb['seqs']], **tb['cfg']) for tb in job['tables']]
    texts, bufs, cuts = [], [], []
    for path in job['texts']:
        text = np.fromfile(path, dtype=np.uint8)
        d = scan.DeviceBuffer(text.nbytes); d.upload(text)
        texts.append(text); bufs.append(d); cuts.append(F.two_batches(text, scan.chunk_offsets(text)))
    depth = job['depth']
    assert depth == len(tables)
    scanners = [scan.Scanner(tables[i], **job['tables'][i].get('options', {})) for i in range(depth)]
    flying = []

    def end():
        k, sc = flying.pop(0)
        r = sc.finish()
        pack(out, 's%d' % k, r, dict(launch_info=sc.launch_info(), scanner=k % depth))

    for k in range(job['steps']):
        sc = scanners[k % depth]
        sc.reset()
        which = (k + k // depth) % len(texts)
        for base, nbytes, co, fpos in cuts[which]:
            sc.scan_device(bufs[which].ptr + base, nbytes, co, fpos_base=fpos)
        sc.finish_begin()
        flying.append((k, sc))
        if len(flying) == depth:
            end()
    while flying:
        end()
    for sc in scanners:
        sc.close()
    for t in tables:
        t.close()
    for d in bufs:
        d.free()


def main(job_path):
    with open(job_path) as f:
        job = json.load(f)
    out = {}
    (rounds if job['kind'] == 'rounds' else ring)(job, out)
    with open(job['result'], 'wb') as f:
        np.savez(f, **out)
    print('inflight child ok: %s' % job['kind'])


if __name__ == '__main__':
    main(sys.argv[1])
