"""``kvarq_amd.options.ScanOptions`` without the library: the flags for kvq_findseqs_opts and the setter calls for a scan handle,
for every on/off combination of the options"""
import itertools

import pytest

from kvarq_amd import _lib
from kvarq_amd.options import ScanOptions


@pytest.mark.parametrize('long_reads', [False, 'auto'])
@pytest.mark.parametrize('rec,prof,cyc,per,dup', itertools.product((False, True), repeat=5))
def test_flags_and_setters(rec, prof, cyc, per, dup, long_reads):
    o = ScanOptions(records=rec, profile='(I' if prof else None, cycles=cyc, per_read=per, duplication=dup, long_reads=long_reads)
    kept, cuts = prof or cyc or per or dup, [40, 73] if prof else []           # (a profile with no cutoffs is implied)
    assert o.profile == (cuts if kept else None)
    f = o.find_opts(2)
    assert f.size == 20 and f.n_cutoffs == len(cuts) and list(f.cutoffs) == cuts + [0] * (8 - len(cuts))
    assert f.flags == (2 | (4 if rec else 0) | (64 if long_reads else 0) |
                       ((8 | (16 if cyc else 0) | (128 if per else 0) | (256 if dup else 0)) if kept else 0))
    calls = [(name, (list(args[0])[:args[1]],) if name == 'kvq_scan_set_profile' else args) for name, args in o.setters()]
    assert calls == ([('kvq_scan_set_records', (1,))] if rec else []) + \
        (([('kvq_scan_set_profile', (cuts,))] + ([('kvq_scan_set_cycles', (1,))] if cyc else []) +
          ([('kvq_scan_set_read_stats', (per + 2 * dup,))] if per or dup else [])) if kept else []) + \
        ([('kvq_scan_set_long_reads', (2,))] if long_reads else [])


def test_refusals():
    for kw, exc in ((dict(long_reads=2), ValueError), (dict(profile=range(9)), ValueError), (dict(profile=['ab']), TypeError), (dict(inflate='host'), TypeError)):
        with pytest.raises(exc):
            ScanOptions(**kw)
    assert _lib.long_reads_mode(True) == ScanOptions(long_reads=True).long_mode == 1
