"""
Scans in flight on an MI355X: kvq_seeded_launch's other order -- the chain published AHEAD of kvq_verify_survivors, which then
runs as KVQ_SV_GRID x 256 threads beside the next scan object's persistent kernel -- against the oracle.

Whether a launch takes that order by itself is timing (was the scan in front still on the device?), so the tests force it
with the switches the launcher documents for that, KVQ_SV_MODE and KVQ_SV_GRID, in child processes (both are read once per
process; tests/inflight_child.py), and every test first asserts from ``Scanner.launch_info()`` and ``match_info()`` that
it got there -- the order, the grid and block of kvq_verify_survivors, more slots than two rounds cover -- and only then
compares the whole result with the oracle's.  The inputs are tests/inflight.py's; tests/test_inflight_host.py holds
their properties.  What was measured: profiles/inflight_tests.txt.

* rounds: a lone scanner whose workgroups walk the round loop of kvq_verify_survivors three times and more (64 x 256), dozens
  and hundreds of times (3 x 256, 1 x 256); a list cut to 100 slots, a failed speculation, an arena that overflows
  in a later round, and -- one scan workgroup, one survivors' workgroup -- whole rounds that emit nothing.
* the ring: three scanners with three different tables take turns on three different texts as bench.py's do, every
  step compared with the answer of its own (table, text) pair, under both forced orders and left to itself.
"""
import bisect
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import inflight as F
import profile_ref as R
from kvarq_amd import scan
from kvarq_amd.engine import Hit
from test_gpu_kernel_matrix import CHILD_LIMIT, compare
from test_gpu_records import split_records

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'inflight_child.py')
# the switches the children are run under; everything else of the environment is the parent's
OURS = ('KVQ_SV_MODE', 'KVQ_SV_GRID', 'KVQ_GRID', 'KVQ_SURV_CAP', 'KVQ_ARENA_CAP')
BESIDE = {'sv64': dict(KVQ_SV_MODE='1'), 'sv1': dict(KVQ_SV_MODE='1', KVQ_SV_GRID='1'), 'sv3': dict(KVQ_SV_MODE='1', KVQ_SV_GRID='3')}
BEHIND = dict(KVQ_SV_MODE='0')
SV_GRID = {'sv64': F.SV_GRID_BESIDE, 'sv1': 1, 'sv3': 3}
CUTS = R.CUTOFFS8
STEPS, DEPTH = 9, 3


def run_child(tmp_path, job, env, what):
    """the .npz one child wrote.  A child is a GPU step of its own with a time limit of its own; one that ends by a signal,
    aborts, runs into the limit or reports an illegal memory access ends the session: nothing more is started on the GPU
    behind it, and nothing is tried again (the rule of tests/test_gpu_kernel_matrix.py)"""
    res, path = str(tmp_path / 'result.npz'), str(tmp_path / 'job.json')
    with open(path, 'w') as f:
        json.dump(dict(job, result=res), f)
    full = dict((k, v) for k, v in os.environ.items() if k not in OURS)
    full.update(env)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, path], env=full, capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as e:
        pytest.exit('%s, %s: the child did not end within %d s\n%s\n%s' % (what, env, CHILD_LIMIT, e.stdout, e.stderr), 1)
    print('%s, %s: child took %.1f s' % (what, env, time.time() - t0))
    said = p.stdout + p.stderr
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
        pytest.exit('%s, %s: the child ended with status %d\n%s' % (what, env, p.returncode, said), 1)
    assert p.returncode == 0 and 'inflight child ok' in p.stdout, (what, env, said)
    return np.load(res)


def load(z, prefix):
    """what Scanner.finish gave, from the child's arrays"""
    a = lambda name: z['%s_%s' % (prefix, name)]
    off, blob = a('offsets').tolist(), a('blob').tobytes()
    cols = [a(c).tolist() for c in ('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')]
    r = dict(hits=tuple(Hit(*h) for h in zip(*cols)), hitseqs=[blob[x:y] for x, y in zip(off[:-1], off[1:])],
             stats=dict(nseqhits=tuple(a('nseqhits').tolist()), nseqbasehits=tuple(a('nseqbasehits').tolist()),
                        readlengths=tuple(a('readlengths').tolist()), records_parsed=int(a('records_parsed'))),
             coverage=a('coverage'), mutations=a('mutations'))
    r.update(json.loads(str(a('meta'))))
    if prefix + '_rec_blob' in z:
        off, blob = a('rec_offsets').tolist(), a('rec_blob').tobytes()
        r['records'] = [blob[x:y] for x, y in zip(off[:-1], off[1:])]
    if prefix + '_profile' in z:
        r['profile'] = a('profile'); r['profile_cutoffs'] = a('profile_cutoffs').tolist()
    return r


def write_texts(tmp_path, texts):
    files = []
    for i, text in enumerate(texts):
        files.append(str(tmp_path / ('t%d.fastq' % i)))
        np.asarray(text).tofile(files[-1])
    return files


def group(table, files):
    _, seqs, cfg = table
    return dict(seqs=[q.decode('latin-1') for q in seqs], cfg=cfg, texts=files)


def went_beside(r, sv_grid, what, launches=None):
    """the scan's seed-filter launches all published ahead of their survivors, verified by sv_grid x 256 threads"""
    li = r['launch_info']
    assert li['launches'] >= 1 and li['beside'] == li['launches'] and li['last_beside'], (what, li)
    assert launches is None or li['launches'] == launches, (what, li)
    assert (li['sv_grid'], li['sv_block']) == (sv_grid, F.SV_BLOCK_BESIDE), (what, li)
    return li


def walked_rounds(r, what, rounds=3):
    """... and the list held more slots than `rounds` - 1 rounds of that launch cover: some workgroup walked `rounds`"""
    li, mi = r['launch_info'], r['match_info']
    per = li['sv_grid'] * li['sv_block']
    assert mi['survivors_cap'] == 1 << 22 and mi['survivors'] > (rounds - 1) * per, (what, mi, per)
    most, fewest = F.rounds_per_workgroup(mi['survivors'], li['sv_grid'], li['sv_block'])
    assert most >= rounds, (what, most)
    print('%s: %d slots, %d x %d threads: %d..%d rounds a workgroup; launches %d, beside %d' % (
        what, mi['survivors'], li['sv_grid'], li['sv_block'], fewest, most, li['launches'], li['beside']))


def mtbc_oracle(text):
    _, seqs, cfg = F.tables()[0]
    return F.oracle_of(text, seqs, cfg)


_memo = {}


def crowded_oracle():
    if 'crowded' not in _memo:
        _memo['crowded'] = mtbc_oracle(F.crowded_text())
    return _memo['crowded']


def dense_oracle():
    if 'dense' not in _memo:
        _memo['dense'] = mtbc_oracle(F.dense_text())
    return _memo['dense']


@pytest.mark.parametrize('sv', sorted(BESIDE))
def test_workgroups_that_walk_the_survivors_in_many_rounds(sv, tmp_path):
    """the dense text (every read a hit on several diagonals) and, through the same scanner behind it, the first text of
    the families; then a table and a text whose speculated record split fails validation (the generator of
    test_a_failed_speculation_redoes_the_whole_batch_on_every_feed): kvq_verify_survivors returns at its first line and the
    batch is redone as a whole"""
    import test_gpu_parity as TP
    _, qtext, qseqs, qo = TP._quirk_case(0, every=True)
    files = write_texts(tmp_path, [F.dense_text(), F.texts()[0], qtext])
    job = dict(kind='rounds', groups=[group(F.tables()[0], files[:2]), group(('quirk', qseqs, TP.QUIRK_CFG), files[2:])])
    z = run_child(tmp_path, job, BESIDE[sv], 'rounds')
    dense, small, quirk = load(z, 'g0t0'), load(z, 'g0t1'), load(z, 'g1t0')
    went_beside(dense, SV_GRID[sv], 'dense', launches=1)
    walked_rounds(dense, 'dense ' + sv)
    compare(dense, dense_oracle(), 'dense ' + sv, min_hits=10000)
    went_beside(small, SV_GRID[sv], 'families 0', launches=1)
    compare(small, F.families()[0, 0], 'families 0 ' + sv)
    went_beside(quirk, SV_GRID[sv], 'quirk', launches=1)
    assert quirk['path']['rescanned'] is True, quirk['path']
    compare(quirk, qo, 'quirk ' + sv)


@pytest.mark.parametrize('sv', sorted(BESIDE))
def test_a_list_cut_to_a_hundred_slots_ends_a_round_in_mid_wave(sv, tmp_path):
    """KVQ_SURV_CAP=100: n = 100 is no multiple of the chunk (16), of the wave (64) or of the block (256): the second wave of
    workgroup 0 holds 36 slots; what found no room is verified in place"""
    files = write_texts(tmp_path, [F.texts()[2]])
    z = run_child(tmp_path, dict(kind='rounds', groups=[group(F.tables()[0], files)]), dict(BESIDE[sv], KVQ_SURV_CAP='100'), 'cut list')
    r = load(z, 'g0t0')
    went_beside(r, SV_GRID[sv], 'cut list', launches=1)
    mi = r['match_info']
    assert mi['survivors_cap'] == 100 and mi['survivors'] >= 100, mi
    assert 100 % 16 and 100 % 64 and 100 % (SV_GRID[sv] * 256)
    compare(r, F.families()[0, 2], 'cut list ' + sv)


@pytest.mark.parametrize('sv', sorted(BESIDE))
def test_an_arena_that_overflows_in_a_later_round_is_grown_and_the_scan_replayed(sv, tmp_path):
    """KVQ_ARENA_CAP = three quarters of the text's hits, and more than the first rounds of all workgroups together can emit: they
    look at sv_grid x 256 slots, and a slot emits two hits at the most (hitAB and hitC).  Every hit comes from that kernel (the
    whole table is in the seed index), so the arena runs over in a later round: arena_at + at then passes arena_cap for the
    rest of the kernel, workgroup by workgroup.  The library grows the arena and replays the batch.  (The dense text for 1 and 3
    workgroups; 64 need the crowded text for that bound: 32 768 hits are more than the dense text has)"""
    text, o = (F.crowded_text(), crowded_oracle()) if sv == 'sv64' else (F.dense_text(), dense_oracle())
    cap = len(o['hits']) * 3 // 4
    assert 2 * SV_GRID[sv] * F.SV_BLOCK_BESIDE < cap < len(o['hits'])
    files = write_texts(tmp_path, [text])
    z = run_child(tmp_path, dict(kind='rounds', groups=[group(F.tables()[0], files)]), dict(BESIDE[sv], KVQ_ARENA_CAP=str(cap)), 'small arena')
    r = load(z, 'g0t0')
    went_beside(r, SV_GRID[sv], 'small arena', launches=2)          # (the replay launches again)
    walked_rounds(r, 'small arena ' + sv)
    assert r['arena_cap_before'] == cap and r['order_info']['arena_cap'] >= len(o['hits']) > cap, (r['order_info'], cap)
    assert r['path']['rescanned'] is False
    compare(r, o, 'small arena ' + sv, min_hits=10000)


def test_rounds_that_emit_nothing_between_rounds_that_do(tmp_path):
    """KVQ_GRID=1, KVQ_SV_GRID=1: one scan workgroup hands out the list's chunks in the order in which it takes the tiles -- F.draw_order,
    not the order of the text; F.silent_text lays the near-miss tiles out as one run of it --, one workgroup of 256 walks them.  The
    stretch's records, scanned alone, say how many slots near-misses take; F.silent_rounds turns that into the whole rounds that find
    no hit at all (total == 0: the third barrier of the round is skipped) between rounds that do"""
    text, cls, stretch, order = F.silent_text()
    files = write_texts(tmp_path, [text, stretch])
    env = dict(BESIDE['sv1'], KVQ_GRID='1')
    z = run_child(tmp_path, dict(kind='rounds', groups=[group(F.tables()[0], files)]), env, 'silent')
    whole, alone = load(z, 'g0t0'), load(z, 'g0t1')
    for r, what in ((whole, 'silent text'), (alone, 'its stretch alone')):
        li = went_beside(r, 1, what, launches=1)
        assert r['grid'] == 1 and (li['grid_cap'], li['grid_cap_kind']) == (1, 'KVQ_GRID'), (what, r['grid'], li)
    slots = alone['match_info']['survivors']
    silent = F.silent_rounds(slots)
    print('silent stretch: its records alone %d slots, at least %d silent rounds of 256; the whole text %d slots' % (slots, silent, whole['match_info']['survivors']))
    assert silent >= 2, (slots, silent)
    walked_rounds(whole, 'silent text', rounds=silent + 2)
    o = mtbc_oracle(text)
    of = [int(cls[h.file_pos // F.RB]) for h in o['hits']]
    assert set(of) == {F.HEAD, F.TAIL} and min(of.count(F.HEAD), of.count(F.TAIL)) >= 500
    compare(whole, o, 'silent text', min_hits=1000)
    compare(alone, mtbc_oracle(stretch), 'its stretch alone', min_hits=0)
    assert len(alone['hits']) == 0


def test_the_large_workgroups_behind_the_scan_walk_several_rounds_too(tmp_path):
    """KVQ_SV_MODE=0, the order of a job that runs alone: 256 x 1024 threads, a round of 262 144 slots.  The crowded text -- a dozen
    hits a read -- fills more than two such rounds"""
    files = write_texts(tmp_path, [F.crowded_text()])
    z = run_child(tmp_path, dict(kind='rounds', groups=[group(F.tables()[0], files)]), BEHIND, 'crowded')
    r = load(z, 'g0t0')
    li = r['launch_info']
    assert li['launches'] == 1 and li['beside'] == 0 and not li['last_beside'], li
    assert (li['sv_grid'], li['sv_block']) == (F.SV_GRID_BEHIND, F.SV_BLOCK_BEHIND), li
    walked_rounds(r, 'crowded text')
    compare(r, crowded_oracle(), 'crowded text', min_hits=10 * F.CROWD_RECORDS)


def test_launch_info_counts_from_the_first_launch_and_from_a_reset():
    """all zeros while the scan object has had no seed-filter launch: fresh, after a reset, and when the exhaustive kernels
    did everything; a job that runs alone finds no scan in front of it"""
    _, seqs, cfg = F.tables()[0]
    t = scan.Table(seqs, **cfg)
    s = scan.Scanner(t)
    zero = dict(zip(scan.Scanner.LAUNCH_INFO, [0] * 10), grid_cap_kind=None, last_beside=False)
    assert s.launch_info() == zero
    s.scan_host(F.texts()[0])
    r = s.finish()
    li = s.launch_info()
    assert li['launches'] == 1 and li['pipelined'] == 0 and li['cus'] > 0 and li['live_scans'] >= 1, li
    assert r['grid'] <= li['grid_cap'] and li['grid_cap_kind'] == ('KVQ_GRID' if int(os.environ.get('KVQ_GRID') or 0) else 'grid_full'), (r['grid'], li)
    if not os.environ.get('KVQ_SV_MODE'):
        assert li['beside'] == 0 and not li['last_beside'] and (li['sv_grid'], li['sv_block']) == (F.SV_GRID_BEHIND, F.SV_BLOCK_BEHIND), li
    compare(r, F.families()[0, 0], 'alone')
    s.reset()
    assert s.launch_info() == zero
    s.force_exhaustive()
    s.scan_host(F.texts()[0])
    r = s.finish()
    assert r['path']['seeded'] is False and s.launch_info() == zero
    s.close(); t.close()


# ---------------------------------------------------------------------------------------------------------------
# the ring
# ---------------------------------------------------------------------------------------------------------------

def ring_job(tmp_path):
    files = write_texts(tmp_path, F.texts())
    tabs = []
    for i, (_, seqs, cfg) in enumerate(F.tables()):
        tabs.append(dict(seqs=[q.decode('latin-1') for q in seqs], cfg=cfg, options=dict(records=True, profile=CUTS) if i == 0 else {}))
    return dict(kind='ring', tables=tabs, texts=files, steps=STEPS, depth=DEPTH)


_profiles = {}


def check_step(z, k, what):
    """step k against the oracle's answer for its own (table, text) pair; -> its launch_info"""
    r = load(z, 's%d' % k)
    table, which = k % DEPTH, (k + k // DEPTH) % len(F.texts())
    assert r['scanner'] == table
    compare(r, F.families()[table, which], (what, 'step', k, 'table', table, 'text', which))
    if table == 0:
        text = F.texts()[which].tobytes()
        recs = split_records(text)
        b0 = [x[1] for x in recs]
        assert len(r['records']) == len(r['hits'])
        for h, rec in zip(r['hits'], r['records']):
            a, lo, hi, e = recs[bisect.bisect_right(b0, h.file_pos) - 1]
            assert lo <= h.file_pos < hi and rec == text[a:e], (what, k, h)
        if which not in _profiles:
            _profiles[which] = R.profile(text, CUTS, [int(x) for x in scan.chunk_offsets(F.texts()[which])])
        assert r['profile_cutoffs'] == CUTS and (r['profile'] == _profiles[which]).all(), (what, k)
        R.check_identities(r['profile'], len(CUTS))
    else:
        assert 'records' not in r and 'profile' not in r
    li = r['launch_info']
    assert li['launches'] == 2 and li['live_scans'] == DEPTH and li['grid_cap_kind'] in ('grid_full', 'grid_shared'), (what, k, li)
    assert li['grid_cap'] == 4 * li['cus'] - (li['cus'] // 4 if li['grid_cap_kind'] == 'grid_shared' else 0), (what, k, li)
    return li


@pytest.mark.parametrize('order', sorted(BESIDE) + ['behind'])
def test_three_scanners_three_tables_three_texts_in_flight(order, tmp_path):
    """nine steps, three in flight: step k is scanner k % 3 (its own table) on text (k + k // 3) % 3, so that every scanner meets
    every text and is used again behind a different one.  Forced beside: every launch publishes ahead of its survivors (the
    next scanner's kernel may start while this one's survivors, validation, redo, fold, records, profile and tail still
    run); forced behind: none does.  The same inputs, the same nine answers: the two orders agree"""
    env = BESIDE[order] if order in BESIDE else BEHIND
    z = run_child(tmp_path, ring_job(tmp_path), env, 'ring')
    for k in range(STEPS):
        li = check_step(z, k, 'ring ' + order)
        if order in BESIDE:
            assert li['beside'] == 2 and li['last_beside'] and (li['sv_grid'], li['sv_block']) == (SV_GRID[order], F.SV_BLOCK_BESIDE), (k, li)
        else:
            assert li['beside'] == 0 and not li['last_beside'] and (li['sv_grid'], li['sv_block']) == (F.SV_GRID_BEHIND, F.SV_BLOCK_BEHIND), (k, li)
    print('ring %s: pipelined launches per step %s' % (order, [load(z, 's%d' % k)['launch_info']['pipelined'] for k in range(STEPS)]))


def test_the_ring_left_to_itself(tmp_path):
    """nothing set: the launcher decides by what it finds on the device.  How many launches go beside is timing and is not
    asserted (profiles/inflight_tests.txt has what an MI355X did); that the answers are the oracle's and that the report is
    consistent -- beside exactly where pipelined, 64 x 256 exactly where beside -- is"""
    z = run_child(tmp_path, ring_job(tmp_path), {}, 'ring')
    seen = []
    for k in range(STEPS):
        li = check_step(z, k, 'ring, nothing set')
        assert li['beside'] == li['pipelined'] <= li['launches'], (k, li)
        assert (li['sv_grid'], li['sv_block']) == ((F.SV_GRID_BESIDE, F.SV_BLOCK_BESIDE) if li['last_beside'] else (F.SV_GRID_BEHIND, F.SV_BLOCK_BEHIND)), (k, li)
        assert li['beside'] > 0 or not li['last_beside']
        seen.append((li['beside'], li['grid_cap_kind']))
    print('ring, nothing set: (launches beside of 2, grid cap) per step %s' % seen)
