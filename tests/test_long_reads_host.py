"""
The texts of tests/long_reads.py say what they claim (no GPU): the oracle reports every alignment their builders planted --
each class, each family with each subset of its blocks broken, each seam -- exactly as often as planted, the flood read has
more candidates than the kernel's queue holds, and every text stays small.
"""
import pytest

import long_reads as LR


@pytest.mark.parametrize('name', LR.NAMES)
def test_the_oracle_finds_what_the_builder_planted(name):
    T = LR.text(name)
    assert len(T.text) < LR.SIZE_CAP and T.want
    assert T.geo is not None and T.geo['seeded']
    LR.check_wanted(T, LR.oracle(name)['hits'])


def test_every_family_and_block_subset_is_planted():
    for name, e in (('classes', 2), ('k6', 3), ('k5', 1)):
        labels = {label for label, _, _ in LR.text(name).want}
        for broken in LR.subsets_of_blocks(e):
            for fam in ('S', 'H/B', 'H/C', 'T'):
                assert '%s broken %s' % (fam, broken,) in labels
        assert {'A overlap %d' % ov for ov in (LR.text(name).cfg['minoverlap'], LR.text(name).cfg['minoverlap'] + 1, 59)} <= labels
        assert sum(n == 2 for _, _, n in LR.text(name).want) == 2           # the B/C duplicates
    assert LR.subsets_of_blocks(2) == [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]
    labels = {label for label, _, _ in LR.text('seams').want}
    assert len([l for l in labels if l.startswith('walk seam')]) == 24 and len([l for l in labels if l.startswith('lane seam')]) == 16
    assert max(h[4] for _, h, _ in LR.text('huge').want) == 200000 and min(h[2] for _, h, _ in LR.text('huge').want) < -65535
    assert [LR.text('stride_%d' % n).geo['stride'] for n in (25, 27, 30, 31)] == [2, 4, 4, 8]
    assert (LR.text('k6').geo['K'], LR.text('k5').geo['K'], LR.text('classes').geo['K']) == (6, 5, 8)
    assert LR.text('with_n').geo['seeded'] == [0, 2]


def test_the_flood_read_overflows_the_queue():
    T = LR.text('flood')
    n = LR.anchor_candidates(T.flood_read, T.seqs, T.geo)
    assert n == 2500 > 4 * LR.QUEUE
    assert len(LR.oracle('flood')['hits']) > 9000
