"""
The generated cases of tests/fuzz_passes.py on an MI355X: hostile files (ragged reads, stray bytes, CR LF, score lines of another
length, truncated tails, malformed records, with planted adapters, near-misses and repeated records in front) through every input
pass and every route.  Every pass on one ``engine.findseqs`` call against the oracle and the plain statements; the adapter clip
against the oracle and the plain statements on the masked text; the BGZF, gzip and BAM routes; the read-list route on the seeded
cases; ``scan.Scanner`` under chunk cuts and batch cuts of the test's choosing, with a replay after an arena overflow.  Every
quantity is an integer or a byte string: the comparisons are exact.  tests/test_fuzz_passes_host.py asserts on the CPU what the
slice reaches and that the references agree among themselves on it.

Four more legs take the emit, its deflate and the tolerant adapter probes through the same files: ``emit=`` on ``findseqs`` beside
every pass, beside the tolerant clip, deflated, and on the read-list route; the emit on the BGZF, gzip and BAM routes, with the
BGZF it wrote read back in on the device-inflate route; ``Scanner(emit=True)`` under the cuts of the scanner leg, deflated on
every other feeding, with the arena replay, and the tokens of a deflated member against ``deflate_ref.parse``;
``adapter_mismatches=`` against the Hamming loop of ``adapt_mm_ref``, in the content pass, the clip and a ``Scanner`` batch.

The cases come in NGROUPS groups of about 15 (the four newer legs, whose references take longer: NGROUPS_NEW groups of 5), a leg and a group a test.  A test ends by asserting that what the leg compared --
cases, hits, refusals, files of every route -- is what the references say of its group (``fuzz_passes.expected``), so a leg that
left something out fails in the group where it did; the host test asserts that those figures, summed over the groups, reach the
floors of ``fuzz_passes.LEG_FLOORS``.  No test depends on another having run.
``python tests/fuzz_passes.py FIRST COUNT [seeded]`` runs the same legs over any seed range.
"""
import collections

import pytest

import fuzz_passes as Z

pytestmark = pytest.mark.gpu

LEGS = dict(Z.LEGS)
BROKEN = []                                                    # an error that is no mismatch (the runtime's, HIP's): nothing more runs on the device


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv('KVQ_ARENA_CAP', raising=False)


@pytest.mark.parametrize('leg,group', [pytest.param(name, i, id='%s-%d' % (name, i)) for name, _ in Z.LEGS for i in range(Z.ngroups(name))])
def test_generated_cases(leg, group, tmp_path, monkeypatch):
    assert not BROKEN, 'not run: an earlier case ended in an error of the runtime, %s' % BROKEN[0]
    tally = collections.Counter()
    cases = Z.group(group, Z.ngroups(leg))
    for seed, seeded in cases:
        if leg == 'long_reads' and not seeded:
            continue
        c, r = Z.case(seed, seeded), Z.refs(seed, seeded)
        for name, value in Z.environ(c).items():
            monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
        try:
            LEGS[leg](c, r, tmp_path, tally)
        except AssertionError as e:
            raise AssertionError('seed %d (%s), cfg %r, %d probes, %d cutoffs: %s' % (seed, 'seeded' if seeded else 'general', c.cfg, len(c.probes), len(c.cuts), e))
        except Exception as e:
            BROKEN.append('seed %d (%s), leg %s: %r' % (seed, 'seeded' if seeded else 'general', leg, e))
            raise
    want = Z.expected(leg, cases)
    print(leg, group, dict(tally))
    for key in set(want) | (set(tally) - {'read list', 'hits of the BAM'}):
        assert tally[key] == want[key], (key, tally[key], want[key])


def test_the_read_list_route_has_its_cases():
    """``leg_long_reads`` requires of every case that the route ran exactly where the table has a seed index; here: it has one in
    at least 30 accepted seeded cases of the slice"""
    assert not BROKEN, 'not run: an earlier case ended in an error of the runtime, %s' % BROKEN[0]
    accepted = [s for s in Z.slice_() if s[1] and Z.refs(*s).accepted]
    assert sum(Z.table_is_seeded(Z.case(*s)) for s in accepted) >= 30
