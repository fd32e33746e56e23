"""The pivot pick of the decode chain on packed rows of layout 2 (htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2;
its `finish` takes the dword of three inside the group of twelve with a two-level search, and its `issue` takes the group
with the top field's compare as the borrow of a subtraction).  A wrong select shows only on the slots m that reach it, so
the inputs here are built to reach every one: every (group g, pivot rank q, rank r inside the dword) that an alphabet has,
the first and the last slot of a symbol under every q, m == 0, and m equal to the root's top field.

Streams are made by the CPU oracle and decoded by rans4x16_hip_uncompress_dev_sized; the decoded bytes are compared with
the RAW INPUT, never with output of the code under test, and every case asserts its route as l1 (the options of
test_gpu_dec_shadow.py).  Every stream has 256 zero bytes behind it, as test_gpu_dec_trip16.py pads, so that the 16-step
trips run up to the last steps; the 8-step loop (fast and slow trips) finishes every stream with the same step.

A case is 15 streams of one alphabet, n = 13, 24, 25, 36, 37, 46, 48 symbols (order 1, 10-bit tables), byte values
0 .. n - 1: byte 0 is a symbol like the others here, so the rows in which it has a frequency have first = 0 and an
alphabet of n symbols reaches all n ranks - with 48 symbols the rank 47, whose end is the top field of D4, the dword
behind the last group.  Stream i holds
  * a walk that takes every ordered pair of two symbols once (every symbol in every context);
  * a hub symbol H_i followed 1,100 times by one of a few `wide` symbols, one per group of twelve, and back: the context
    H_i is seen more than 1,024 times, which compute_shift normalises to 1,024 with 10 bits - the successors seen once in
    the walk get frequency 1 beside wide ones of about 270 in every group, so m equals the first AND the last slot of the
    symbol whenever one of them is decoded; symbol 0 after H_i is m == 0, symbol 36 (or the last symbol, under 37
    symbols, where the top field is the 1023 of "beyond the end") is m equal to the root's top field;
  * uniform draws from the other symbols up to its length of 4 to 5 KiB plus 0 .. 7 bytes.
The model of test_dec_pivot_cpu.py decodes the same streams (checked against the raw input) and says what they reach;
the GPU test asserts that coverage before it trusts the GPU run.  No triple is left out for any alphabet.

Waves: DEC_CLASSES gives 13 symbols sixteen streams per wave, 48 symbols thirteen, the others fifteen or sixteen; a wave
holds streams of ONE class.  So the mix of a 48-symbol stream with 13-symbol streams runs in one call but in launches
of their own (the classifier cannot put them into one wave), and the wave that does mix alphabets is of 36 and 37
symbols, which share a class: 36 = 3 x 12 symbols have the dword L[36 ..] behind their last group (D4 selectable), 37
have not (their D4 of group 3 is the next row's first dword)."""
import functools

import numpy as np
import pytest

import test_dec_pivot_cpu as P
import test_gpu_dec_shadow as S
from test_gpu_dec_step import H, check_route, decode, device, mismatches, stream_info  # noqa: F401
from test_gpu_dec_trip16 import PAD

ALPHABETS = (13, 24, 25, 36, 37, 46, 48)
WAVE = 15
VISITS = 1100
OPTS = S.OPTS


# ---- generators ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_pairs(n):
    """An Euler circuit of the complete digraph with loops on n symbols: every ordered pair once."""
    nxt = {h: list(range(n)) for h in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == n * n + 1 and len(set(zip(circuit, circuit[1:]))) == n * n
    return circuit


def hub_of(n, i):
    return (5 * i + 1) % n


def wide_of(n, i):
    w = [s for s in range((5 + i) % 12, n, 12) if s != hub_of(n, i)]
    return w or [(hub_of(n, i) + 1) % n]


def length_of(n, i):
    return max(4096, (n * n + 1 + 2 * VISITS + 512 + 1023) // 1024 * 1024) + i % 8


@functools.lru_cache(maxsize=None)
def stream(n, i):
    """(name, raw, stream + PAD zero bytes)."""
    import cpu_libs
    rng = np.random.default_rng(1000 * n + i)
    hub, wide = hub_of(n, i), wide_of(n, i)
    seq = list(all_pairs(n))
    for v in range(VISITS):
        seq += [hub, wide[v % len(wide)]]
    others = np.array([v for v in range(n) if v != hub])      # (the hub's row stays what the walk and the visits made it)
    seq += others[rng.integers(0, n - 1, size=length_of(n, i) - len(seq))].tolist()
    raw = np.array(seq, dtype=np.uint8).tobytes()
    return ("n%d/%d" % (n, i), raw, cpu_libs.oracle().compress(raw, 1) + bytes(PAD))


def wave_of(n):
    return [stream(n, i) for i in range(WAVE)]


# ---- the model: what the streams reach ----------------------------------------------------------------------------
def table_of(s):
    """(stream_info, decoded size, symbols, {context: frequencies of 1,024}, offset of the four states) of a stream."""
    info = stream_info(s)
    assert info.coded and info.order == 1 and info.bits == 10, info
    size, pos = S._varint(s, 1)
    if info.nested:                                         # the table travels as an order-0 stream
        import cpu_libs
        usz, pos = S._varint(s, pos + 1)
        csz, pos = S._varint(s, pos)
        src = np.frombuffer(s[pos:pos + csz], dtype=np.uint8)
        tab = np.zeros(usz + 16, dtype=np.uint8)
        assert cpu_libs.oracle().lib.orc_o0_decode(src.ctypes.data, csz, tab.ctypes.data, usz) == 0
        syms, freqs, _ = S._o1_freqs(tab.tobytes(), 0, 10)
        pos += csz
    else:
        syms, freqs, pos = S._o1_freqs(s, pos + 1, 10)
    return info, size, syms, freqs, pos


@functools.lru_cache(maxsize=None)
def reached(n, i):
    """The stream decoded with the layout-2 look-up (two-level pick) of test_dec_pivot_cpu.py: (decoded bytes, the set
    of (g, q, r, m is the symbol's first slot, m is its last slot, m == 0, m == the root's top field) of its steps)."""
    _, _, s = stream(n, i)
    info, size, syms, freqs, pos = table_of(s)
    assert info.nsym == n
    assert pos + 16 == info.words and syms.tolist() == list(range(n))
    rows = {c: P.build_row(f.tolist()) for c, f in freqs.items() if f.sum()}
    x = [int(v) for v in np.frombuffer(s[pos:pos + 16], dtype="<u4")]
    words = np.frombuffer(s[info.words:info.words + 2 * info.nwords], dtype="<u2").tolist()
    q = size >> 2
    out = bytearray(size)
    ctx, at, seen, memo = [0, 0, 0, 0], 0, set(), {}
    for t in range(q + (size & 3)):
        for k in (range(4) if t < q else (3,)):
            m = x[k] & 1023
            hit = memo.get((ctx[k], m))
            if hit is None:
                root, leaf, first, _ = rows[ctx[k]]
                _, _, pq, g, r, sym, freq, off = P.lookup(root, leaf, first, m, P.pick2)
                hit = memo[(ctx[k], m)] = (sym, freq, off, (g, pq, r, off == 0, off == freq - 1, m == 0, root >> 22 == m))
            sym, freq, off, what = hit
            seen.add(what)
            x[k] = freq * (x[k] >> 10) + off
            ctx[k] = sym
            out[k * q + t] = sym
            if x[k] < (1 << 15) and at < len(words):
                x[k] = (x[k] << 16) | words[at]
                at += 1
    assert at <= info.nwords - PAD // 2                    # a well-formed stream never asks for the padding
    return bytes(out), frozenset(seen)


def triples_of(n):
    """Every (g, q, r) that an alphabet of n symbols has: the ranks 0 .. n - 1 of a row whose first symbol is byte 0."""
    return {(c // 12, c % 12 // 3, c % 3) for c in range(n)}


LEFT_OUT = {n: set() for n in ALPHABETS}                   # triples that cannot be reached, with the reason: none


def assert_coverage(n):
    seen = set()
    for i in range(WAVE):
        out, what = reached(n, i)
        assert out == stream(n, i)[1], (n, i)              # the model decodes the stream: its steps are the chain's
        seen |= what
    assert {w[:3] for w in seen} == triples_of(n) - LEFT_OUT[n], (n, sorted(triples_of(n) - {w[:3] for w in seen}))
    for q in {t[1] for t in triples_of(n)}:
        assert any(w[1] == q and w[3] for w in seen) and any(w[1] == q and w[4] for w in seen), (n, q)
        assert any(w[1] == q and w[3] and not w[4] for w in seen) and any(w[1] == q and w[4] and not w[3] for w in seen), (n, q)
    assert any(w[5] for w in seen) and any(w[6] for w in seen), n
    if n == 48:
        assert (3, 3, 2) in {w[:3] for w in seen}          # cur is the top field of D4
    return seen


# ---- GPU ----------------------------------------------------------------------------------------------------------
def run(dc, items, shifts=None):
    what = [name for name, _, _ in items]
    raws = [raw for _, raw, _ in items]
    st, osz, got, route, _ = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    check_route(route, {"l1": len(items)})


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALPHABETS)
def test_every_pivot_of_the_alphabet(H, opts, n):
    assert_coverage(n)
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    run(dc, wave_of(n), shifts=[(3 * i + n) % 16 for i in range(WAVE)])


@pytest.mark.gpu
def test_alphabets_side_by_side(H, opts):
    """One 48-symbol stream with fourteen 13-symbol streams in one call (two classes: launches of their own), and a wave
    that alternates 36 and 37 symbols (one class: the D4 of a 36-symbol row's last group is its own dword L[36 ..], that
    of a 37-symbol row's group 3 the next row's first dword)."""
    for n in (13, 36, 37, 48):
        assert_coverage(n)
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    run(dc, [stream(48, 0)] + [stream(13, i) for i in range(14)])
    run(dc, [stream(36 + (i & 1), i) for i in range(WAVE)], shifts=[(7 * i + 2) % 16 for i in range(WAVE)])


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALPHABETS)
def test_cases_are_what_they_claim(n):
    """No GPU.  Coded, order 1, n symbols, 10 bits (asserted by `reached`); 4 to 16 KiB; the hub's row holds frequency 1
    beside wide symbols in every group of twelve; the coverage the GPU test relies on; the 16-step trips run."""
    from test_gpu_dec_trip16 import ENTRY_WORDS
    from test_gpu_routes import _expected_level
    assert _expected_level(n, 0, 0) == "l1"
    seen = assert_coverage(n)
    for name, raw, s in wave_of(n):
        assert 4096 <= len(raw) <= 16384 and set(raw) == set(range(n)), name
        assert stream_info(s).nwords - PAD // 2 >= 4 * ENTRY_WORDS, name
    # stream 0's hub row, from the stream's own table
    freqs = table_of(stream(n, 0)[2])[3]
    f = freqs[hub_of(n, 0)]
    for g in range((n + 11) // 12):
        part = f[12 * g:12 * g + 12]
        assert part.min() == 1 and (part.max() >= 100 or len(part) < 6), (n, g, part.tolist())
    print(n, "steps reach", len(seen), "kinds; triples", len({w[:3] for w in seen}))
