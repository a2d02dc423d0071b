"""
The generated cases of tests/fuzz_passes.py on the CPU: the slice reaches what it is built for (floors counted from the plain
statements and the oracle alone: no kernel can make them true or false), and on every case the CPU twins of the passes equal the
plain statements, the identities of every reference module hold, the clip is idempotent, and the oracle parses as many records of
the masked text as of the text as it lies.  The same for the emit, its deflate and the tolerant probes: the draws that were there
have not moved (a digest), the twins of the emit, the tolerant content and the tolerant clip equal their plain statements, every
emitted text a leg deflates passes ``deflate_ref.check``, and a census of its own has its floors (profiles/fuzz_emit_tests.txt).
tests/test_gpu_fuzz_passes.py runs the same cases on an MI355X.
"""
import numpy as np
import pytest

import adapt_mm_ref as AM
import clip_ref as CR
import deflate_ref as D
import emit_ref as E
import fuzz_passes as Z
import profile_ref as R
from kvarq_amd import profile as P
from oracle import oracle as O


def test_the_slice_is_what_its_rule_gives():
    assert Z.slice_() == Z.slice_by_rule()


def test_the_slice_reaches_what_it_is_built_for():
    n = Z.census()
    print(dict(n))
    for key, floor in Z.FLOORS.items():
        assert n[key] >= floor, (key, n[key], floor)
    assert n['cases'] == n['accepted'] + n['refused'] == len(Z.slice_()) == sum(len(Z.group(i)) for i in range(Z.NGROUPS))
    assert all(10 <= len(Z.group(i)) <= 20 for i in range(Z.NGROUPS))
    assert sum(1 for s in Z.slice_() if len(Z.case(*s).text) > Z.CHUNK) == 2
    # the draws cover what they are drawn from
    cases = [Z.case(*s) for s in Z.slice_()]
    assert {len(c.cuts) for c in cases} == {0, 1, 2, 4, 5, 8} and {c.dup_slots for c in cases} == {None, 64, 1024}
    assert {c.over_records for c in cases} == {None, 50, 1000} and {len(p) for c in cases for p in c.probes} >= set(Z.PROBE_LENGTHS)
    assert all(1 <= len(c.probes) <= 8 and len(set(c.probes)) == len(c.probes) for c in cases)
    assert sum(1 for c in cases if c.cfg['Amin'] == '!') >= 1            # (the clip's refusal has a case)


def test_the_draws_that_were_there_have_not_moved():
    """``emit_min`` and ``per`` come from a stream of their own: text, sequences, configuration, probes, cutoffs and table sizes of
    every case of the slice are what they were before the two were drawn"""
    assert Z.slice_digest() == Z.SLICE_DIGEST
    assert Z.NGROUPS == 8 and all(Z.ngroups(leg) == (Z.NGROUPS_NEW if leg in Z.NEW_LEGS else Z.NGROUPS) for leg, _ in Z.LEGS)
    assert sum(len(Z.group(i, Z.NGROUPS_NEW)) for i in range(Z.NGROUPS_NEW)) == len(Z.slice_())


def test_the_slice_reaches_the_emit_and_the_tolerant_probes():
    n = Z.emit_census()
    print(dict(n))
    for key, floor in list(Z.EMIT_FLOORS.items()) + list(Z.TOLERANT_FLOORS.items()):
        assert n[key] >= floor, (key, n[key], floor)
    for key in ['emit_min %r' % (m,) for m in Z.EMIT_MINS] + ['per %d' % p for p in Z.PERS]:
        assert n[key] >= 10, (key, n[key])
    accepted = len(Z.slice_()) - n['refused']
    assert 4 * n['adapters differ'] >= accepted and 4 * n['mask differs'] >= accepted, (n['adapters differ'], n['mask differs'], accepted)
    # a floor is three quarters of what is there, or more
    for key, floor in Z.TOLERANT_FLOORS.items():
        assert 4 * floor >= 3 * n[key] - 3, (key, floor, n[key])
    assert Z.LEG_FLOORS['tolerant']['tolerant hits'] >= n['FIRST at distance >= 1: records']


@pytest.mark.parametrize('leg', sorted(Z.LEG_FLOORS))
def test_no_leg_of_the_gpu_test_is_vacuous(leg):
    """the GPU test requires of every group that a leg's tally is ``expected`` of the group; summed over the groups those reach the
    floors: hits, a refused case per file route, cases per route"""
    assert set(Z.LEG_FLOORS) == {name for name, _ in Z.LEGS}
    groups = [Z.expected(leg, Z.group(i, Z.ngroups(leg))) for i in range(Z.ngroups(leg))]
    whole = Z.expected(leg, Z.slice_())
    assert sum(groups, Z.collections.Counter()) == +whole
    print(leg, dict(whole))
    for key, floor in Z.LEG_FLOORS[leg].items():
        assert whole[key] >= floor, (leg, key, whole[key], floor)


@pytest.mark.parametrize('group', range(Z.NGROUPS))
def test_twins_equal_the_plain_statements(group):
    for seed, seeded in Z.group(group):
        c, r = Z.case(seed, seeded), Z.refs(seed, seeded)
        what = 'seed %d (%s)' % (seed, 'seeded' if seeded else 'general')
        if not r.accepted:
            continue
        text, probes = c.text, list(c.probes)
        assert len(r.recs) == r.outcome[3]['records_parsed'], what           # the plain statement's records are the oracle's
        twin = P.profile_host(text, list(c.cuts), r.co, cycles=True, per_read=True, duplication=True, slots=c.dup_slots or 0, overrepresented=True,
                              over_records=c.over_records or 0, adapters=probes)
        Z.same_passes(twin, r.passes, what + ': the twin')
        r.passes.check_identities(c, text)
        masked, words = (r.masked, r.clip_words) if r.masked is not None else CR.mask(text, r.co, probes)
        once, w1 = P.clip_host(text, probes, r.co)
        assert bytes(once) == masked and (w1 == words).all(), what + ': clip_host'
        twice, w2 = P.clip_host(once, probes, r.co)
        assert bytes(twice) == masked and w2[CR.C_RECORDS] == w1[CR.C_RECORDS] and w2[CR.C_CLIPPED] == w1[CR.C_CLIPPED], what + ': the clip twice'
        assert len(masked) == len(text) and R.records_of(masked, r.co) == r.recs
        o = r.masked_outcome if r.masked_outcome is not None else Z.oracle_outcome(masked, c.seqs, c.cfg)
        assert o[0] == 'ok' and o[3]['records_parsed'] == r.outcome[3]['records_parsed'], what + ': the oracle on the masked text'
        if r.masked_passes is not None:
            r.masked_passes.check_identities(c, masked)
            assert (r.masked_passes.adapt == r.passes.adapt).all() and (r.masked_passes.cycles[Z.CY.CYCLES * 256:] == r.passes.cycles[Z.CY.CYCLES * 256:]).all()


@pytest.mark.parametrize('group', range(Z.NGROUPS))
def test_twins_of_the_emit_and_the_tolerant_probes_equal_the_plain_statements(group):
    """the emit's twin at the drawn ``emit_min`` and at None, on the text and on the tolerantly masked text; the emit under a merged
    cut is its batches one behind the other; the tolerant twins of content and clip against the Hamming loop; the clip twice is
    the clip once; and every emitted text a leg compares in its deflated form passes ``deflate_ref.check`` by the deflate's twin"""
    for seed, seeded in Z.group(group):
        c, r = Z.case(seed, seeded), Z.refs(seed, seeded)
        what = 'seed %d (%s)' % (seed, 'seeded' if seeded else 'general')
        if not r.accepted:
            continue
        text, probes, amin = c.text, list(c.probes), c.cfg['Amin']
        # the tolerant probes
        assert (P.adapt_host(text, probes, r.co, adapter_mismatches=c.per).words == r.tolerant).all(), what + ': adapt_host, 1 per %d' % c.per
        AM.check_identities(r.tolerant)
        masked, words = (r.masked_mm, r.clip_words_mm) if ord(amin) > ord('!') else AM.mask(text, r.co, probes, c.per)
        once, w1 = P.clip_host(text, probes, r.co, adapter_mismatches=c.per)
        assert bytes(once) == masked and (w1 == words).all(), what + ': clip_host, 1 per %d' % c.per
        twice, w2 = P.clip_host(once, probes, r.co, adapter_mismatches=c.per)
        assert bytes(twice) == masked and w2[AM.C_RECORDS] == w1[AM.C_RECORDS] and w2[AM.C_CLIPPED] == w1[AM.C_CLIPPED], what + ': the tolerant clip twice'
        assert len(masked) == len(text) and R.records_of(masked, r.co) == r.recs
        if ord(amin) > ord('!'):
            assert r.masked_mm_outcome[0] == 'ok' and r.masked_mm_outcome[3]['records_parsed'] == r.outcome[3]['records_parsed'], what
            r.masked_mm_passes.check_identities(c, masked)
            assert (r.masked_mm_passes.adapt == r.tolerant).all()          # (the mask writes score lines only)
        # the emit
        for t, which in [(text, 'the text')] + ([(masked, 'the masked text')] if ord(amin) > ord('!') else []):
            for m in sorted({Z.min_length(c), Z.min_length(c, None)}):
                want, ewords = r.emit_of(t, r.co, m)
                out, w = P.emit_host(t, amin, m, r.co)
                assert out.tobytes() == want and (w == ewords).all(), '%s: emit_host on %s, min_length %d' % (what, which, m)
                E.check_identities(ewords, len(want))
        if len(r.recs) >= 2:
            (whole,), halves = Z.scanner_batches(c, r)
            half = halves[0][1]
            merged = r.emit_of(text, sorted(set(r.co) | {half}))
            parts, pwords = r.emit_batches(text, halves)
            assert merged[0] == b''.join(parts) and (merged[1] == pwords).all(), what + ': the emit under a merged cut'
        # the deflate
        for batch in Z.deflated_batches(c, r):
            out, dwords = Z.twin(batch)
            D.check(out, batch, dwords, deep=2)
            assert Z.bgzf_of([batch]) == out + D.EOF


def test_refused_cases_are_refused_the_same_once_masked():
    same = other = 0
    for seed, seeded in Z.slice_():
        c, r = Z.case(seed, seeded), Z.refs(seed, seeded)
        if r.accepted:
            continue
        masked, _ = CR.mask(c.text, [0, len(c.text)], list(c.probes))
        o = Z.oracle_outcome(masked, c.seqs, c.cfg)
        assert o[0] == 'format', (seed, o[0])
        same += o == r.outcome; other += o != r.outcome
        print('seed %d: %r; masked: %r' % (seed, r.outcome[1], o[1]))
    assert same + other >= 1
