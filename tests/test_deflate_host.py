"""
The emit's deflate without a GPU (include/kvarq_hip.h): the CPU twin kvq_deflate_bgzf_host -- the definition in
running code, over the kvq_deflate.h the kernel runs too -- on the texts of tests/deflate_ref.py, each with its census; the
length-limited code builder on its own against a plain statement of the same rule; the options; and the twin as a program of its
own under AddressSanitizer and UBSan.
"""
import contextlib
import ctypes as C
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import clip_ref as CR
import deflate_ref as D
import emit_ref as E
from kvarq_amd import _lib, options, profile as P

HERE = os.path.dirname(os.path.abspath(__file__))


def emitted(name):
    """EMIT of one of emit_ref's or clip_ref's texts: what the deflate is there for"""
    text = {'copies': lambda: E.copies_text()[0], 'trims': lambda: E.trims_text()[0], 'counts': lambda: E.counts_text(65537),
            'reveal': lambda: CR.reveal_text()[0]}[name]()
    out, _ = P.emit_host(text, E.AMIN, 0, [0, len(text)])
    return out.tobytes()


@pytest.mark.parametrize('name', D.NAMES)
def test_the_twin_on_every_text(name):
    D.text_census(name)
    text = D.text(name)
    out, words = P.deflate_bgzf_host(text)
    assert len(out) == words[D.BYTES_OUT] <= _lib.lib().kvq_deflate_bound(len(text)) and words[D.BYTES_IN] == len(text)
    toks = D.check(out, text, words)
    D.stream_census(name, toks, words.tolist())
    # the same text twice gives the same bytes
    again, words2 = P.deflate_bgzf_host(text)
    assert again == out and (words2 == words).all()


def stream_and_parse(text):
    """[(the tokens of a BTYPE-2 member of the twin's stream, the tokens ``deflate_ref.parse`` gives its block)]"""
    out, _ = P.deflate_bgzf_host(text)
    pairs, at = [], 0
    for _, _, payload, _, isize in D.members(out):
        if (payload[0] >> 1) & 3 == 2:
            pairs.append((D.tokens(payload)['tokens'], D.parse(text[at:at + isize])))
        at += isize
    return pairs


@pytest.mark.parametrize('name', D.NAMES)
def test_the_parse_as_stated_in_python(name):
    """the rule of the parse that kvq_deflate.h states in words, as ``deflate_ref.parse``: the tokens of every BTYPE-2 member are
    the rule's, one for one -- not only within its limits (``check_tokens``)"""
    pairs = stream_and_parse(D.text(name))
    # fifteen members in all: a member of one byte is stored, as are those of 'random'
    assert len(pairs) == {'empty': 0, 'one': 0, 'random': 0, 'two-blocks+1': 2, 'one-byte': 2, 'block-end': 2}.get(name, 1)
    for got, want in pairs:
        assert got == want


def test_the_parse_on_the_emitted_text_of_generated_cases():
    """the first member of the emitted text of every case of group 0 of tests/fuzz_passes.py"""
    import fuzz_passes as Z
    n = 0
    for seed, seeded in Z.group(0):
        c, r = Z.case(seed, seeded), Z.refs(seed, seeded)
        if not r.accepted:
            continue
        text = r.emit_of(c.text, r.co, c.cfg['minreadlength'])[0][:D.BLOCK]
        for got, want in stream_and_parse(text):
            assert got == want, seed
            n += 1
    assert n >= 10


def test_the_eof_member_and_the_bound():
    L = _lib.lib()
    assert P.bgzf_eof() == D.EOF and L.kvq_deflate_len() == D.LEN
    assert [L.kvq_deflate_bound(n) for n in (0, 1, D.BLOCK, D.BLOCK + 1)] == [0, 32, D.BLOCK + 31, D.BLOCK + 1 + 62] and L.kvq_deflate_bound(-1) == -1
    # a buffer one byte short is refused
    text = D.text('random')
    out, _ = P.deflate_bgzf_host(text)
    with pytest.raises(RuntimeError):
        P.deflate_bgzf_host(text, cap=len(out) - 1)
    assert P.deflate_bgzf_host(text, cap=len(out))[0] == out


@pytest.mark.parametrize('name', ['copies', 'trims', 'counts', 'reveal'])
def test_emitted_fastq_takes_dynamic_blocks(name):
    """on FastQ as the emit makes it every full block is BTYPE 2, and shorter than half its text"""
    text = emitted(name)
    out, words = P.deflate_bgzf_host(text)
    toks = D.check(out, text, words, deep=2)
    full = len(text) // D.BLOCK
    assert all(t['btype'] == 2 for t in toks[:full]) and (words[D.STORED] == 0 or full == 0)
    if name == 'counts':
        assert full >= 2 and words[D.BYTES_OUT] < len(text) // 2
        # ... and the yardstick: zlib at level 1 on the same blocks
        z1 = sum(len(zlib.compress(text[i:i + D.BLOCK], 1)) - 6 + 26 for i in range(0, len(text), D.BLOCK))
        print('counts: %d bytes -> %d (twin), %d (zlib level 1)' % (len(text), words[D.BYTES_OUT], z1))


def test_batches_cut_at_a_block_edge_give_the_same_members():
    text = D.text('two-blocks+1')
    whole, w = P.deflate_bgzf_host(text)
    a, wa = P.deflate_bgzf_host(text[:D.BLOCK])
    b, wb = P.deflate_bgzf_host(text[D.BLOCK:])
    assert a + b == whole and (wa + wb)[:6].tolist() == w[:6].tolist() and np.maximum(wa, wb)[6:].tolist() == w[6:].tolist()
    # ... and cut anywhere else they do not
    a, _ = P.deflate_bgzf_host(text[:D.BLOCK - 1])
    b, _ = P.deflate_bgzf_host(text[D.BLOCK - 1:])
    assert a + b != whole and D.check(a + b[:0], text[:D.BLOCK - 1]) is not None


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


HISTOGRAMS = {
    'fibonacci': (fib(22), 15), 'fibonacci-286': ([min(x, 1 << 30) for x in fib(44)] + [1] * 242, 15), 'flat': ([7] * 286, 15), 'one': ([0] * 40 + [9] + [0] * 245, 15),
    'two': ([0, 3, 0, 0, 1000000], 15), 'all-286': (list(range(1, 287)), 15), 'cl-19': ([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181], 7),
    'cl-flat': ([1] * 19, 7), 'none': ([0] * 30, 15), 'sparse': ([0, 5, 0, 5, 0, 0, 1, 0, 2] * 30, 15),
}


@pytest.mark.parametrize('name', sorted(HISTOGRAMS))
def test_the_length_limited_codes(name):
    freq, limit = HISTOGRAMS[name]
    lens = P.deflate_lengths_host(freq, limit).tolist()
    used = [s for s, f in enumerate(freq) if f]
    assert all((lens[s] > 0) == (freq[s] > 0) for s in range(len(freq))) and all(1 <= lens[s] <= limit for s in used)
    if len(used) >= 2:
        assert D.kraft(lens, limit) == 1 << limit                # exactly one
    elif len(used) == 1:
        assert lens[used[0]] == 1                                # the legal one-code case
    want = D.lengths(freq, limit)
    cost = lambda l: sum(f * x for f, x in zip(freq, l))
    assert cost(lens) <= cost(want) and lens == want
    if name in ('fibonacci', 'fibonacci-286', 'cl-19'):
        # the limit acts: the unlimited tree is deeper
        assert max(D.lengths(freq, 60)) > limit == max(lens)
    if name == 'fibonacci':
        assert max(D.lengths(freq, 60)) == 21


def test_the_builder_refuses_what_it_cannot_code():
    L = _lib.lib()
    f = np.ones(19, dtype=np.uint32); lens = np.zeros(19, dtype=np.uint8)
    assert L.kvq_deflate_lengths_host(f.ctypes.data, 19, 4, lens.ctypes.data) == _lib.ERR_RUNTIME       # 19 symbols, 16 codes
    assert L.kvq_deflate_lengths_host(f.ctypes.data, 19, 16, lens.ctypes.data) == _lib.ERR_RUNTIME
    assert L.kvq_deflate_lengths_host(f.ctypes.data, 289, 15, lens.ctypes.data) == _lib.ERR_RUNTIME
    assert L.kvq_deflate_lengths_host(None, 19, 7, lens.ctypes.data) == _lib.ERR_RUNTIME
    big = np.full(19, 1 << 28, dtype=np.uint32)                  # the counts sum to 2^32 and more: the tree's weights would wrap
    assert L.kvq_deflate_lengths_host(big.ctypes.data, 19, 7, lens.ctypes.data) == _lib.ERR_RUNTIME
    assert L.kvq_deflate_lengths_host(big.ctypes.data, 15, 7, lens.ctypes.data) == 0
    assert L.kvq_deflate_lengths_host(f.ctypes.data, 19, 5, lens.ctypes.data) == 0 and D.kraft(lens.tolist(), 5) == 32


def test_the_crc_operators_against_zlib():
    """the members' CRC-32 is put together from the segments' (kvq_crc_shift, kvq_crc_mul): zlib has verified it on every text
    above; here on lengths around the segment and the block"""
    rng = np.random.RandomState(3)
    for n in (1, 2, 254, 255, 256, 509, 510, 511, 65024, 65025, 65026, 65279, 65280):
        text = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        out, _ = P.deflate_bgzf_host(text)
        assert [m[3] for m in D.members(out)] == [zlib.crc32(text)]


def test_the_options():
    o = options.ScanOptions(emit='x.gz')
    assert o.emit_compress is False and ('kvq_scan_set_emit_compress', (1,)) not in o.setters()       # the suffix decides nothing
    assert not o.find_opts().m.a.base.flags & _lib.FIND_EMIT_BGZF
    o = options.ScanOptions(emit=True, emit_compress=True)
    assert o.emit_compress is True and [c[0] for c in o.setters()][-2:] == ['kvq_scan_set_emit', 'kvq_scan_set_emit_compress']
    o = options.ScanOptions(emit='out.fastq', emit_compress=True, emit_min=0)
    f = o.find_opts().m.a.base.flags
    assert f & _lib.FIND_EMIT and f & _lib.FIND_EMIT_BGZF and _lib.FIND_EMIT_BGZF == 16384
    assert options.ScanOptions(emit=True, emit_compress=False).emit_compress is False and options.ScanOptions(emit_compress=False).emit_compress is False
    for bad in (dict(emit_compress=True), dict(emit=True, emit_compress=1), dict(emit=True, emit_compress='yes'), dict(emit=False, emit_compress=True)):
        with pytest.raises(ValueError):
            options.ScanOptions(**bad)


def test_the_flag_without_the_emit_is_refused():
    L = _lib.lib()
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_EMIT_BGZF, 0, (C.c_uint8 * 8)())
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_EMIT' in _lib.last_error()[1]


def test_the_command_line(tmp_path, monkeypatch):
    seen = []

    class Z(dict):
        pass

    def fake(fnames, cutoffs=True, inflate='host', sources=None, **more):
        seen.append(more)
        p = P.profile_host(b'@r\nACGT\n+\nIIII\n', [ord('.')])
        p.emitted = P.Emit(np.array([0, 1, 1, 0, 0, 4, 4, 15], dtype=np.int64))
        p.emit_compressed = P.deflate_words([1, 15, 46, 1, 0, 15, 0, 0]) if more.get('emit_compress') else None
        return p
    monkeypatch.setattr(P, 'profile', fake)
    (tmp_path / 't.fastq').write_bytes(b'@r\nACGT\n+\nIIII\n')
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--emit', str(tmp_path / 'o.gz'), '--emit-bgzf'])
    assert seen[-1]['emit_compress'] is True and 'emit bgzf: members=1 stored=1 bytes 15 -> 74' in out.getvalue()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--emit', str(tmp_path / 'o.gz')])
    assert 'emit_compress' not in seen[-1] and 'emit bgzf' not in out.getvalue()
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        P.main([str(tmp_path / 't.fastq'), '--emit-bgzf'])


def test_twin_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """tests/deflate_twin_main.cpp, built with -fsanitize=address,undefined: the text in a heap block of exactly its size, the output
    in one of exactly kvq_deflate_bound bytes; the program's output is BGZF(text) and the eight words, those of the loaded library"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no C++ compiler'
    exe = str(tmp_path / 'deflate_twin_main')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(HERE, 'deflate_twin_main.cpp')], check=True, capture_output=True, timeout=300)
    for name in ('empty', 'one', 'block', 'block+1', 'one-byte', 'random', 'fibonacci', 'block-end', 'farthest'):
        text = D.text(name)
        (tmp_path / 'in.bin').write_bytes(text)
        p = subprocess.run([exe, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, (name, p.returncode, p.stderr[-2000:])
        got = (tmp_path / 'out.bin').read_bytes()
        want, words = P.deflate_bgzf_host(text)
        assert got[:-64] == want and (np.frombuffer(got[-64:], dtype=np.int64) == words).all(), name
