"""
CPU checks of the test-side DEFLATE tools (tests/deflate_writer.py) and of the structured corpus built
with them (inflate_corpus.edge_valid / edge_invalid): zlib and the reference inflater agree on every
member, each invalid member fails for the rule it was built to break, and the census proves that the
corpus reaches every edge it names.  The library itself is not needed here.
"""
import random
import zlib

import pytest

import deflate_writer as W
import inflate_corpus as IC

EDGE_VALID = IC.edge_valid()
EDGE_INVALID = IC.edge_invalid()


@pytest.mark.parametrize('name,payload,text,features', EDGE_VALID, ids=[m[0] for m in EDGE_VALID])
def test_edge_valid_member_inflates_to_its_text(name, payload, text, features):
    assert len(text) <= 65536
    assert IC.zlib_verdict(payload, len(text)) == (True, text)
    ok, got, why, census = W.inflate(payload, len(text))
    assert (ok, why) == (True, None) and got == text
    for f in features:
        assert IC.EDGE_FEATURES[f](census), (name, f)


@pytest.mark.parametrize('name,payload,isize,reason', EDGE_INVALID, ids=[m[0] for m in EDGE_INVALID])
def test_edge_invalid_member_is_refused_for_its_rule(name, payload, isize, reason):
    assert IC.zlib_verdict(payload, isize) == (False, None)
    ok, got, why, _ = W.inflate(payload, isize)
    assert (ok, got) == (False, None)
    assert why == reason


def test_census_hits_every_named_edge():
    hit, merged = {}, {'max_dist': 0, 'single': 0}
    for name, payload, text, features in EDGE_VALID:
        _, _, _, c = W.inflate(payload, len(text))
        for f, pred in IC.EDGE_FEATURES.items():
            if pred(c):
                hit.setdefault(f, name)
        merged['max_dist'] = max(merged['max_dist'], c['max_dist'])
        merged['single'] += c['single_dist_used']
    missing = sorted(set(IC.EDGE_FEATURES) - set(hit))
    assert not missing, missing
    assert merged['max_dist'] == 32768 and merged['single'] > 0
    declared = set(f for m in EDGE_VALID for f in m[3])
    assert declared == set(IC.EDGE_FEATURES)                  # every edge has a member built for it
    print('\n'.join('%-24s %s' % (f, hit[f]) for f in sorted(hit)))


def test_edge_invalid_corpus_covers_every_rule():
    reasons = set(m[3] for m in EDGE_INVALID)
    assert reasons == {'too many length or distance symbols', 'incomplete code lengths set', 'over-subscribed code lengths set',
                       'empty code lengths set', 'repeat with no first length', 'too many lengths', 'missing end-of-block',
                       'incomplete literal/length code', 'over-subscribed literal/length code', 'over-subscribed distance code',
                       'incomplete distance code', 'invalid code', 'distance too far back', 'isize', 'truncated'}


def test_reference_inflater_equals_zlib_on_the_valid_corpus():
    for label, payload, text in IC.valid_corpus():
        ok, got, why, _ = W.inflate(payload, len(text))
        assert ok and got == text, (label, why)


def test_reference_inflater_verdict_equals_zlib_on_the_corrupt_corpus():
    corpus = IC.corrupt_corpus()
    for i, (p, isize) in enumerate(corpus):
        ok, want = IC.zlib_verdict(p, isize)
        rok, got, why, _ = W.inflate(p, isize)
        assert rok == ok, (i, why)
        assert got == want, i


def test_reference_inflater_equals_zlib_on_libdeflate_members():
    corpus = IC.libdeflate_corpus()
    if corpus is None:
        pytest.skip('libdeflate does not load on this machine')
    far = 0
    for label, payload, text in corpus:
        assert IC.zlib_verdict(payload, len(text)) == (True, text), label
        ok, got, _, c = W.inflate(payload, len(text))
        assert ok and got == text, label
        far = max(far, c['max_dist'])
    assert far > 32506                                        # beyond anything zlib writes


def test_huffman_lengths_are_complete_and_limited():
    rnd = random.Random(3)
    for n, limit in ((286, 15), (30, 15), (19, 7), (2, 15)):
        for _ in range(20):
            fib = [1, 1]
            while len(fib) < n:
                fib.append(fib[-1] + fib[-2])
            freqs = fib[:n] if rnd.random() < 0.3 else [rnd.choice([0, 0, 1, 5, 100, 10000]) for _ in range(n)]
            lens = W.huffman_lengths(freqs, limit)
            used = [s for s in range(n) if freqs[s]]
            if not used:
                assert not any(lens)
                continue
            assert all(lens[s] for s in used) and max(lens) <= limit
            assert sum(2.0 ** -l for l in lens if l) == 1.0


def test_writer_round_trips_random_block_lists():
    for seed in range(30):
        r = random.Random(seed)
        blocks, o = [], 0
        for _ in range(r.randint(1, 5)):
            kind = r.choice(['fixed', 'dynamic', 'stored'])
            if kind == 'stored':
                n = r.choice([0, 1, 50, 3000])
                blocks.append(dict(kind=kind, data=bytes(r.getrandbits(8) for _ in range(n)))); o += n
                continue
            toks = []
            for _ in range(r.randint(0, 600)):
                if o and r.random() < 0.4:
                    ln = r.randint(3, 258)
                    toks.append((ln, r.randint(1, min(o, 32768)), 284) if ln == 258 and r.random() < 0.5 else
                                (ln, r.randint(1, min(o, 32768)))); o += ln
                else:
                    toks.append(r.getrandbits(8)); o += 1
            blocks.append(dict(kind=kind, tokens=toks))
        payload, text = W.build(blocks)
        assert zlib.decompressobj(-15).decompress(payload) == text, seed
        assert W.inflate(payload, len(text))[:2] == (True, text), seed


def test_far_tokens_reach_the_whole_window_and_round_trip():
    text = IC.fastq_text(60000, seed=9)
    toks = W.far_tokens(text)
    assert max(t[1] for t in toks if not isinstance(t, int)) == 32768
    payload, got = W.build([dict(kind='dynamic', tokens=toks)])
    assert got == text and IC.zlib_verdict(payload, len(text)) == (True, text)
