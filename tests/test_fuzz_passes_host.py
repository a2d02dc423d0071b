"""
The generated cases of tests/fuzz_passes.py on the CPU: the slice reaches what it is built for (floors counted from the plain
statements and the oracle alone: no kernel can make them true or false), and on every case the CPU twins of the passes equal the
plain statements, the identities of every reference module hold, the clip is idempotent, and the oracle parses as many records of
the masked text as of the text as it lies.  tests/test_gpu_fuzz_passes.py runs the same cases on an MI355X.
"""
import numpy as np
import pytest

import clip_ref as CR
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


@pytest.mark.parametrize('leg', sorted(Z.LEG_FLOORS))
def test_no_leg_of_the_gpu_test_is_vacuous(leg):
    """the GPU test requires of every group that a leg's tally is ``expected`` of the group; summed over the groups those reach the
    floors: hits, a refused case per file route, cases per route"""
    assert set(Z.LEG_FLOORS) == {name for name, _ in Z.LEGS}
    groups = [Z.expected(leg, Z.group(i)) for i in range(Z.NGROUPS)]
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
