"""Inputs and expected results of the cross-codec best-of tests (test_best_any_cpu.py, test_gpu_best_any.py; include/
rans4x16_hip.h part 2m).  The expectations come from the CPU alone: cpu_libs.oracle() for rANS 4x16 and
arith_enc_model.compress for arith_dynamic, each pinned to the reference by its own suite.  No test lives here."""
import functools
import os

import numpy as np

import arith_enc_model as AE
import arith_model as AM
import cpu_libs

CODEC_RANS, CODEC_ARITH, CODEC_MASK = 0, 1 << 24, 0x0F000000
OK, CAPACITY, SIZE, UNSUPPORTED, EMPTY = 0, 1, 5, 6, 9
X_STRIPE = 8
HERE = os.path.dirname(os.path.abspath(__file__))
R4X16_GOLDEN = os.path.join(HERE, "golden", "r4x16")

SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 16, 20, 21, 24, 32, 64, 100, 256, 1000, 4096)
ALPHABETS = (1, 2, 4, 6, 45, 256)
ORDERS = (0, 1, 64, 65, 128, 129, 192, 193, 8, 9)
TEXTS = ("q4", "q8", "q40+dir", "qvar")


def rans(order):
    return CODEC_RANS | order


def arith(order):
    return CODEC_ARITH | order


@functools.lru_cache(maxsize=None)
def _rans_stream(data, order):
    return cpu_libs.oracle().compress(data, order)


@functools.lru_cache(maxsize=None)
def _arith_stream(data, order):
    return AE.compress(data, order)


def skipped(size, method):
    """tokenise_name3.c:1270: a stripe method is not tried on a size that is no multiple of 4"""
    return bool(method & X_STRIPE) and size % 4 != 0


def pick(size, methods, stream_of):
    """What block of `size` bytes gets under the tagged list `methods`, given stream_of(tagged method) -> bytes:
    (chosen tagged method or -1, stream or None, status, tie).  Per codec the first smallest of the methods that are tried;
    across codecs the smaller, on equal sizes the one whose winner stands earlier in the list (tie = True)."""
    best = {}
    for pos, m in enumerate(methods):
        tag = m & CODEC_MASK
        assert tag in (CODEC_RANS, CODEC_ARITH)
        best.setdefault(tag, None)
        if skipped(size, m & ~CODEC_MASK):
            continue
        s = stream_of(m)
        if best[tag] is None or len(s) < len(best[tag][1]):
            best[tag] = (pos, s)
    won = [v for v in best.values() if v is not None]
    if not won:
        return -1, None, UNSUPPORTED, False           # every method of the list was skipped
    tie = len(won) == 2 and len(won[0][1]) == len(won[1][1])
    pos, s = min(won, key=lambda v: (len(v[1]), v[0]))
    return methods[pos], s, OK, tie


def expect(data, methods):
    """pick over the CPU encoders"""
    data = bytes(data)

    def stream_of(m):
        order = m & ~CODEC_MASK
        return _arith_stream(data, order) if m & CODEC_MASK == CODEC_ARITH else _rans_stream(data, order)
    return pick(len(data), methods, stream_of)


def text(name):
    return AM.text(name)


@functools.lru_cache(maxsize=None)
def fixture_orders(name):
    """every order word that has a fixture in both tests/golden/r4x16 and tests/golden/arith for text `name`, ascending"""
    def orders(d):
        return {int(f[len(name) + 1:]) for f in os.listdir(d) if f.startswith(name + ".") and f[len(name) + 1:].isdigit()}
    return tuple(sorted(orders(R4X16_GOLDEN) & orders(AM.GOLDEN)))


@functools.lru_cache(maxsize=None)
def fixture_stream(name, method):
    """the reference's own stream for text `name` under the tagged method, from the committed files"""
    d = AM.GOLDEN if method & CODEC_MASK == CODEC_ARITH else R4X16_GOLDEN
    with open(os.path.join(d, "%s.%d" % (name, method & ~CODEC_MASK)), "rb") as f:
        return f.read()


def expect_fixture(name, methods):
    """pick over the committed reference streams of text `name`"""
    return pick(len(text(name)), methods, lambda m: fixture_stream(name, m))


@functools.lru_cache(maxsize=None)
def small_blocks():
    """The small family's blocks, one per (size, alphabet) in that order of loops: RandomState(7), symbols drawn evenly
    from the first `alphabet` byte values."""
    rs = np.random.RandomState(7)
    return tuple(rs.randint(0, a, size=n).astype(np.uint8).tobytes() for n in SIZES for a in ALPHABETS)


@functools.lru_cache(maxsize=None)
def small_family():
    """[(block index, order)]: every block under every order, stripe orders only where the size is a multiple of 4"""
    return tuple((i, o) for i, b in enumerate(small_blocks()) for o in ORDERS if not skipped(len(b), o))


def outcome(data, methods):
    """'rans', 'arith' or 'failed' and whether the sizes were equal, as R4X16_ROUTE_BEST_ANY counts a block"""
    chosen, _, _, tie = expect(data, methods)
    return ("failed" if chosen < 0 else "arith" if chosen & CODEC_MASK == CODEC_ARITH else "rans"), tie


@functools.lru_cache(maxsize=None)
def small_census():
    """Over the small family under the pair list {rANS order, arith order}: (ties, arith wins, rANS wins), the wins with
    different sizes - 693, 276 and 39 with these blocks.  At least 20 of each is a condition, so that the tie rule and both
    directions cannot pass vacuously."""
    ties = a_wins = r_wins = 0
    blocks = small_blocks()
    for i, o in small_family():
        who, tie = outcome(blocks[i], (rans(o), arith(o)))
        assert who != "failed"
        ties += tie
        a_wins += who == "arith" and not tie
        r_wins += who == "rans" and not tie
    assert ties >= 20 and a_wins >= 20 and r_wins >= 20, (ties, a_wins, r_wins)
    return ties, a_wins, r_wins
